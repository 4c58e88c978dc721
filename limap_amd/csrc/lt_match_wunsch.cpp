// lt_match_wunsch.cpp -- the SOLD2 line matcher (limap.line2d.SOLD2: WunschLineMatcher) for a whole scene in one call:
// validation, one upload of the point descriptors and the validity bytes, the launches of lt_kernels_wunsch.hip on the
// context's stream, the rows in the state lt_match_get / lt_match_get_scores / lt_match_get_timers read; and the host
// restatement lt_fn_match_wunsch_pair_host of the same semantics (std::fmaf in a plain loop, the pooling and the
// Needleman-Wunsch recurrence of lt_wunsch.h).  The scene path around the tasks and the launches is the one of
// lt_match_scene.h, shared with lt_match.cpp.  DESIGN §17, "SOLD2".

#include "lt_match_scene.h"
#include "lt_wunsch.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

namespace {

int check_config(const lt_match_wunsch_config *cfg, int dim, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (cfg->topk < 0) { msg = "topk is negative"; return 1; }
  if (cfg->topk > LT_MATCH_MAX_TOPK) { msg = "topk above LT_MATCH_MAX_TOPK (64)"; return 1; }
  if (cfg->num_samples < kWunschMinSamples || cfg->num_samples > kWunschMaxSamples) {
    msg = "num_samples outside [2, 8]";
    return 1;
  }
  if (cfg->top_k_candidates < 1 || cfg->top_k_candidates > LT_MATCH_MAX_TOPK) {
    msg = "top_k_candidates outside [1, LT_MATCH_MAX_TOPK (64)]";
    return 1;
  }
  if (dim < 8 || dim > LT_MATCH_MAX_DIM || (dim & 7)) {
    msg = "descriptor width must be a multiple of 8 in [8, 256]";
    return 1;
  }
  return 0;
}

// validity byte per line (bit s = sample s); false when a line has no valid sample
bool pack_masks(const uint8_t *valid, long long n_lines, int S, unsigned char *out) {
  bool ok = true;
  for (long long l = 0; l < n_lines; ++l) {
    unsigned m = 0;
    for (int s = 0; s < S; ++s) m |= (valid[l * S + s] ? 1u : 0u) << s;
    out[l] = (unsigned char)m;
    ok = ok && m != 0;
  }
  return ok;
}

// the masked S x S block of lines (i, j): P[s * S + t]
void block_scores(const float *d1, unsigned m1, const float *d2, unsigned m2, int dim, int S, float *P) {
  for (int s = 0; s < S; ++s)
    for (int t = 0; t < S; ++t)
      P[s * S + t] = (((m1 >> s) & 1u) && ((m2 >> t) & 1u)) ? dot_chain(d1 + (size_t)s * dim, d2 + (size_t)t * dim, dim)
                                                            : -1.0f;
}

float block_line_score(const float *P, int S) {
  float a[8], b[8];
  for (int k = 0; k < 8; ++k) a[k] = b[k] = -1.0f;  // (a slot past S does not count)
  for (int s = 0; s < S; ++s)
    for (int t = 0; t < S; ++t) {
      const float p = P[s * S + t];
      a[s] = t ? wunsch_max(a[s], p) : p;
      b[t] = s ? wunsch_max(b[t], p) : p;
    }
  return wunsch_line_score(wunsch_pool8(a), wunsch_pool8(b));
}

double block_nw(const float *P, int S, bool reversed) {
  switch (S) {
    case 2: return wunsch_nw<2>(P, S, reversed);
    case 3: return wunsch_nw<3>(P, S, reversed);
    case 4: return wunsch_nw<4>(P, S, reversed);
    case 5: return wunsch_nw<5>(P, S, reversed);
    case 6: return wunsch_nw<6>(P, S, reversed);
    case 7: return wunsch_nw<7>(P, S, reversed);
    default: return wunsch_nw<8>(P, S, reversed);
  }
}

// all blocks of a pair: P as (n1, n2, S, S), L as (n1, n2)
void pair_scores(const float *d1, const unsigned char *m1, long long n1, const float *d2, const unsigned char *m2,
                 long long n2, int dim, int S, float *P, float *L) {
#pragma omp parallel for schedule(static)
  for (long long i = 0; i < n1; ++i) {
    float blk[64];
    for (long long j = 0; j < n2; ++j) {
      float *dst = P ? P + (size_t)(i * n2 + j) * S * S : blk;
      block_scores(d1 + (size_t)i * S * dim, m1[i], d2 + (size_t)j * S * dim, m2[j], dim, S, dst);
      if (L) L[i * n2 + j] = block_line_score(dst, S);
    }
  }
}

}  // namespace

extern "C" {

int lt_match_wunsch_scene(lt_ctx *ctx, int n_img, const int64_t *line_off, const int64_t *desc_off, const float *desc,
                          const uint8_t *valid, int dim, const int64_t *pair_off, const int32_t *pair_nb,
                          const lt_match_wunsch_config *cfg, int64_t *n_rows) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *fn = "lt_match_wunsch_scene";
  const std::string who = std::string(fn) + ": ";
  std::string msg;
  if (check_config(cfg, dim, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + msg);
  const int S = cfg->num_samples;
  if (int rc = check_scene(ctx, fn, n_img, {{"line", line_off}, {"descriptor", desc_off}}, pair_off, pair_nb, !desc || !valid,
                           [&](int m) -> const char * {
                             const int64_t n = line_off[m + 1] - line_off[m];
                             if (desc_off[m + 1] - desc_off[m] != n * S)
                               return "an image's descriptor count is not num_samples times its mask rows";
                             return n > kMatchMaxLines ? "more than 65535 lines in an image" : nullptr;
                           }))
    return rc;
  const long long n_lines = line_off[n_img], n_desc = desc_off[n_img], n_pairs = pair_off[n_img];
  std::vector<unsigned char> vmask((size_t)std::max<long long>(n_lines, 1), 0);
  if (!pack_masks(valid, n_lines, S, vmask.data()))
    return fail(ctx, LT_ERR_ARGUMENT, who + "a line has no valid sample");
  double t0 = now_ms();

  // ---- tasks (a pair each; mutual: the swapped pairs behind them), units, output slots ----
  const bool mutual = cfg->topk == 0;
  const int topk = mutual ? cfg->top_k_candidates : cfg->topk;
  std::vector<WunschTask> tasks((size_t)n_pairs * (mutual ? 2 : 1));
  std::vector<int> kk((size_t)n_pairs);  // columns kept per line: the mutual form keeps a line's one match
  std::vector<long long> &row_off = ctx->mt.row_off;
  row_off.assign((size_t)n_pairs + 1, 0);
  long long slots = 0, mslots = 0;
  int kcap = 0;
  {
    long long p = 0;
    for (int m = 0; m < n_img; ++m)
      for (; p < pair_off[m + 1]; ++p) {
        const int nb = pair_nb[p];
        WunschTask &T = tasks[(size_t)p];
        T.a0 = desc_off[m];
        T.b0 = desc_off[nb];
        T.la0 = line_off[m];
        T.lb0 = line_off[nb];
        T.na = (int)(line_off[m + 1] - line_off[m]);
        T.nb = (int)(line_off[nb + 1] - line_off[nb]);
        T.kk = T.na > 0 ? std::min(topk, T.nb) : 0;
        T.out0 = slots;
        T.mout0 = mslots;
        T.pad_ = 0;
        slots += (long long)T.na * T.kk;
        if (T.kk) mslots += T.na;
        row_off[(size_t)p + 1] = mutual ? mslots : slots;  // (mutual: an upper bound, replaced by collect_rows)
        kk[(size_t)p] = mutual ? (T.kk ? 1 : 0) : T.kk;
        kcap = std::max(kcap, T.kk);
      }
  }
  if (mutual)
    for (long long p = 0; p < n_pairs; ++p) {
      const WunschTask &F = tasks[(size_t)p];
      WunschTask &B = tasks[(size_t)(n_pairs + p)];
      B = WunschTask{F.b0, F.a0, F.lb0, F.la0, slots, mslots, F.nb, F.na, F.na > 0 && F.nb > 0 ? std::min(topk, F.na) : 0, 0};
      slots += (long long)B.na * B.kk;
      if (B.kk) mslots += B.na;
      kcap = std::max(kcap, B.kk);
    }
  if (slots >= (1ll << 40)) return fail(ctx, LT_ERR_ARGUMENT, who + "too many result rows");
  const int waves = kWunschMaxWaves;
  std::vector<MatchUnit> units;
  std::vector<long long> prefix(tasks.size() + 1, 0);  // lines of the tasks that match at all, for k_wunsch_nw
  for (size_t t = 0; t < tasks.size(); ++t) {
    prefix[t + 1] = prefix[t] + (tasks[t].kk > 0 ? tasks[t].na : 0);
    if (tasks[t].kk > 0)
      for (int r0 = 0; r0 < tasks[t].na; r0 += kWunschTileLines * waves) units.push_back(MatchUnit{(int)t, r0});
  }
  if (units.size() > 0x7fffffffull) return fail(ctx, LT_ERR_ARGUMENT, who + "too many row tiles");

  // ---- upload ----
  const float *d_desc = nullptr;
  if (int rc = stage_desc(ctx, fn, desc, n_desc * dim, cfg->desc_on_device != 0, &d_desc)) return rc;
  if (int rc = upload_vec(ctx, ctx->mt.d_vmask, vmask)) return rc;
  if (int rc = upload_vec(ctx, ctx->mt.d_tasks, tasks)) return rc;
  if (int rc = upload_vec(ctx, ctx->mt.d_units, units)) return rc;
  if (mutual)
    if (int rc = upload_vec(ctx, ctx->mt.d_prefix, prefix)) return rc;
  ENSURE(ctx, ctx->mt.d_col, 2 * (size_t)std::max<long long>(slots, 1) + 16);
  ENSURE(ctx, ctx->mt.d_score, 4 * (size_t)std::max<long long>(slots, 1));
  if (mutual) {
    ENSURE(ctx, ctx->mt.d_mcol, 2 * (size_t)std::max<long long>(mslots, 1) + 16);
    ENSURE(ctx, ctx->mt.d_mscore, 4 * (size_t)std::max<long long>(mslots, 1));
  }
  if (int rc = stream_sync(ctx)) return rc;
  double t1 = now_ms();
  ctx->mt.timers[0] = t1 - t0;

  // ---- kernels ----
  hipStream_t st = ctx->stream;
  Events<3> ev;
  if (int rc = ev.create(ctx)) return rc;
  const WunschTask *d_tasks = ctx->mt.d_tasks.as<WunschTask>();
  const unsigned char *d_vmask = ctx->mt.d_vmask.as<unsigned char>();
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_wunsch_topk(st, dim, S, kcap, waves, d_tasks, ctx->mt.d_units.as<MatchUnit>(), (int)units.size(), d_desc, d_vmask,
                     ctx->mt.d_col.as<unsigned short>(), ctx->mt.d_score.as<float>());
  if (int rc = ev.record(ctx, 1)) return rc;
  if (mutual) {
    launch_wunsch_nw(st, dim, S, d_tasks, ctx->mt.d_prefix.as<long long>(), (int)tasks.size(), prefix.back(), d_desc,
                     d_vmask, ctx->mt.d_col.as<unsigned short>(), ctx->mt.d_score.as<float>(),
                     ctx->mt.d_mcol.as<unsigned short>(), ctx->mt.d_mscore.as<float>());
    if (int rc = ev.record(ctx, 2)) return rc;
    launch_wunsch_mutual(st, d_tasks, (int)n_pairs, ctx->mt.d_mcol.as<unsigned short>());
  }
  if (int rc = stream_sync(ctx)) return rc;
  double t2 = now_ms();
  ctx->mt.timers[1] = t2 - t1;
  ctx->mt.kernel_ms[0] = ev.ms(0, 1);
  ctx->mt.kernel_ms[1] = mutual ? ev.ms(1, 2) : 0.0;

  // the mutual form's rows are the matches of k_wunsch_nw that survived the cross check, a slot per line
  return collect_rows(ctx, mutual ? ctx->mt.d_mcol : ctx->mt.d_col, mutual ? ctx->mt.d_mscore : ctx->mt.d_score,
                      std::move(kk), cfg->want_scores != 0, mutual, t2, n_rows);
}

int lt_match_wunsch_get_kernel_ms(lt_ctx *ctx, double out[2]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  out[0] = ctx->mt.kernel_ms[0];
  out[1] = ctx->mt.kernel_ms[1];
  return LT_OK;
}

int lt_fn_match_wunsch_scores_host(const float *desc1, const uint8_t *valid1, int64_t n1, const float *desc2,
                                   const uint8_t *valid2, int64_t n2, int dim, int num_samples, float *point_scores,
                                   float *line_scores) {
  lt_match_wunsch_config cfg = {1, num_samples, 1, 0, 0, 0};
  std::string msg;
  if (check_config(&cfg, dim, msg) || n1 < 0 || n2 < 0 || n1 > kMatchMaxLines || n2 > kMatchMaxLines) return LT_ERR_ARGUMENT;
  if ((n1 && (!desc1 || !valid1)) || (n2 && (!desc2 || !valid2))) return LT_ERR_ARGUMENT;
  const int S = num_samples;
  if (!values_ok(desc1, n1 * S * dim) || !values_ok(desc2, n2 * S * dim)) return LT_ERR_ARGUMENT;
  std::vector<unsigned char> m1((size_t)n1 + 1), m2((size_t)n2 + 1);
  if (!pack_masks(valid1, n1, S, m1.data()) || !pack_masks(valid2, n2, S, m2.data())) return LT_ERR_ARGUMENT;
  pair_scores(desc1, m1.data(), n1, desc2, m2.data(), n2, dim, S, point_scores, line_scores);
  return LT_OK;
}

int lt_fn_match_wunsch_nw_host(const float *block, int num_samples, double out[2]) {
  if (!block || !out || num_samples < kWunschMinSamples || num_samples > kWunschMaxSamples) return LT_ERR_ARGUMENT;
  out[0] = block_nw(block, num_samples, false);
  out[1] = block_nw(block, num_samples, true);
  return LT_OK;
}

int lt_fn_match_wunsch_pair_host(const float *desc1, const uint8_t *valid1, int64_t n1, const float *desc2,
                                 const uint8_t *valid2, int64_t n2, int dim, const lt_match_wunsch_config *cfg,
                                 int32_t *rows2, float *scores, int64_t *n_rows) {
  std::string msg;
  if (check_config(cfg, dim, msg) || n1 < 0 || n2 < 0 || !n_rows) return LT_ERR_ARGUMENT;
  if (n1 > kMatchMaxLines || n2 > kMatchMaxLines) return LT_ERR_ARGUMENT;
  if ((n1 && (!desc1 || !valid1)) || (n2 && (!desc2 || !valid2))) return LT_ERR_ARGUMENT;
  const int S = cfg->num_samples;
  if (!values_ok(desc1, n1 * S * dim) || !values_ok(desc2, n2 * S * dim)) return LT_ERR_ARGUMENT;
  std::vector<unsigned char> m1((size_t)n1 + 1), m2((size_t)n2 + 1);
  if (!pack_masks(valid1, n1, S, m1.data()) || !pack_masks(valid2, n2, S, m2.data())) return LT_ERR_ARGUMENT;
  *n_rows = 0;
  if (n1 == 0 || n2 == 0) return LT_OK;
  const bool mutual = cfg->topk == 0;
  std::vector<float> P(mutual ? (size_t)n1 * n2 * S * S : 0), L((size_t)n1 * n2);
  pair_scores(desc1, m1.data(), n1, desc2, m2.data(), n2, dim, S, mutual ? P.data() : nullptr, L.data());
  std::vector<unsigned long long> best;
  long long n = 0;
  if (!mutual) {
    const int kk = (int)std::min<long long>(cfg->topk, n2);
    best_columns(n1, n2, kk, [&](long long i, long long j) { return L[(size_t)(i * n2 + j)]; }, best);
    for (long long i = 0; i < n1; ++i)
      for (int t = 0; t < kk; ++t, ++n) {
        const unsigned long long key = best[(size_t)(i * kk + t)];
        if (rows2) { rows2[2 * n] = (int32_t)i; rows2[2 * n + 1] = (int32_t)match_key_col(key); }
        if (scores) scores[n] = match_key_score(key);
      }
    *n_rows = n;
    return LT_OK;
  }
  // mutual form: per direction the candidates ascending in the key, forward blocks before reversed ones, first maximum
  auto direction = [&](bool swapped, std::vector<int> &match, std::vector<float> &mscore) {
    const long long na = swapped ? n2 : n1, nb = swapped ? n1 : n2;
    const int kc = (int)std::min<long long>(cfg->top_k_candidates, nb);
    best_columns(na, nb, kc, [&](long long i, long long j) { return L[(size_t)(swapped ? j * n2 + i : i * n2 + j)]; }, best);
    match.assign((size_t)na, -1);
    mscore.assign((size_t)na, 0.0f);
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < na; ++i) {
      double best_v = 0.0;
      int best_pos = -1;
      float blk[64];
      for (int pos = 0; pos < 2 * kc; ++pos) {
        const long long j = match_key_col(best[(size_t)(i * kc + (kc - 1 - pos % kc))]);
        const float *src = P.data() + (size_t)((swapped ? j * n2 + i : i * n2 + j)) * S * S;
        for (int s = 0; s < S; ++s)
          for (int t = 0; t < S; ++t) blk[s * S + t] = swapped ? src[t * S + s] : src[s * S + t];
        const double v = block_nw(blk, S, pos >= kc);
        if (best_pos < 0 || v > best_v) { best_v = v; best_pos = pos; }
      }
      const unsigned long long key = best[(size_t)(i * kc + (kc - 1 - best_pos % kc))];
      match[(size_t)i] = (int)match_key_col(key);
      mscore[(size_t)i] = match_key_score(key);
    }
  };
  std::vector<int> f, b;
  std::vector<float> fs, bs;
  direction(false, f, fs);
  direction(true, b, bs);
  for (long long i = 0; i < n1; ++i) {
    if (b[(size_t)f[(size_t)i]] != (int)i) continue;
    if (rows2) { rows2[2 * n] = (int32_t)i; rows2[2 * n + 1] = f[(size_t)i]; }
    if (scores) scores[n] = fs[(size_t)i];
    ++n;
  }
  *n_rows = n;
  return LT_OK;
}

}  // extern "C"
