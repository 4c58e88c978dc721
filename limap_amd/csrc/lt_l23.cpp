// lt_l23.cpp -- 2D-3D line matching for localization (limap_amd.localization): validation, upload, the
// launches of lt_kernels_l23.hip, the one readback that sizes the output, and the download; lt_fn_l23_host is the same
// definition in plain C++ from the same inline functions (lt_l23.h), so both agree bit for bit.  Grouping kept pairs
// into per-line lists in upstream's order (group_rows) is shared by the twin and by the device path's listed modes.

#include "lt_host.h"
#include "lt_l23.h"
#include "lt_twin.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

constexpr const char *kWho = "limap_amd.localization";

struct Plan {
  L23Cfg cfg;
  long long n_db = 0, Q = 0, n_task = 0, n_dbseg = 0, n_qseg = 0, n_units = 0, n_pairs = 0, T = 0;
  std::vector<long long> db_seg_off, q_seg_off, task_off, unit_off, pair_off;
  std::vector<int> task_q;
  bool listed() const { return cfg.mode != kL23AllPairs; }
};

// first k of v[0 .. n) that is not finite, -1 where all are
long long first_non_finite(const double *v, long long n) {
  for (long long k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return k;
  return -1;
}

// The checks of both entry points, in one order.  1 and the message where the input is refused.
int make_plan(const lt_l23_input *in, const lt_l23_config *c, Plan &pl, std::string &msg) {
  if (!in || !c) { msg = "null input or configuration"; return 1; }
  if (c->mode < kL23AllPairs || c->mode > kL23ListedFiltered) { msg = "unknown mode " + std::to_string(c->mode); return 1; }
  if (c->filter < kL23NoFilter || c->filter > kL23MidpointPerpendicular) { msg = "unknown filter kind " + std::to_string(c->filter); return 1; }
  if (std::isnan(c->IoU_threshold) || std::isnan(c->dist_thres) || std::isnan(c->sine_thres) || !std::isfinite(c->angle_scale)) {
    msg = "non-finite threshold or angle_scale";
    return 1;
  }
  pl.cfg = L23Cfg{c->mode, c->filter, c->IoU_threshold, c->dist_thres, c->sine_thres, c->angle_scale};
  const long long lim = INT_MAX;
  if (in->n_db < 0 || in->n_query < 0 || in->n_tracks < 0 || in->n_db > lim || in->n_query > lim || in->n_tracks > lim) {
    msg = "an image, query or track count is negative or above 2^31 - 1";
    return 1;
  }
  pl.n_db = in->n_db; pl.Q = in->n_query; pl.T = in->n_tracks;
  if (pl.n_db > 0 && !in->db_cam11) { msg = "null database cameras"; return 1; }
  if (pl.Q > 0 && !in->q_cam11) { msg = "null query cameras"; return 1; }
  for (const auto &o : {std::make_tuple("database segment", pl.n_db, in->db_seg_off), std::make_tuple("query segment", pl.Q, in->q_seg_off),
                        std::make_tuple("task", pl.Q, in->task_off)}) {
    msg = offsets_msg(std::get<0>(o), std::get<1>(o), std::get<2>(o));
    if (!msg.empty()) return 1;
  }
  pl.n_dbseg = in->db_seg_off[pl.n_db]; pl.n_qseg = in->q_seg_off[pl.Q]; pl.n_task = in->task_off[pl.Q];
  if (pl.n_dbseg > lim || pl.n_qseg > lim || pl.n_task > lim) { msg = "more than 2^31 - 1 segments or tasks"; return 1; }
  if ((pl.n_dbseg > 0 && (!in->db_seg4 || !in->db_track)) || (pl.n_qseg > 0 && !in->q_seg4) || (pl.n_task > 0 && !in->task_db) ||
      (pl.T > 0 && c->filter != kL23NoFilter && !in->track6)) {
    msg = "null segment, task or track arrays";
    return 1;
  }
  if (pl.listed()) {
    msg = offsets_msg("pair", pl.n_task, in->pair_off);
    if (!msg.empty()) return 1;
    pl.n_pairs = in->pair_off[pl.n_task];
    if (pl.n_pairs > lim) { msg = "more than 2^31 - 1 listed pairs"; return 1; }
    if (pl.n_pairs > 0 && !in->pairs2) { msg = "null listed pairs"; return 1; }
  }
  long long k;
  if ((k = first_non_finite(in->db_cam11, 11 * pl.n_db)) >= 0) { msg = "non-finite camera of database image " + std::to_string(k / 11); return 1; }
  if ((k = first_non_finite(in->db_seg4, 4 * pl.n_dbseg)) >= 0) { msg = "non-finite database segment " + std::to_string(k / 4); return 1; }
  if ((k = first_non_finite(in->q_cam11, 11 * pl.Q)) >= 0) { msg = "non-finite camera of query " + std::to_string(k / 11); return 1; }
  if ((k = first_non_finite(in->q_seg4, 4 * pl.n_qseg)) >= 0) { msg = "non-finite query segment " + std::to_string(k / 4); return 1; }
  if (c->filter != kL23NoFilter && (k = first_non_finite(in->track6, 6 * pl.T)) >= 0) { msg = "non-finite track " + std::to_string(k / 6); return 1; }
  pl.db_seg_off.assign(in->db_seg_off, in->db_seg_off + pl.n_db + 1);
  pl.q_seg_off.assign(in->q_seg_off, in->q_seg_off + pl.Q + 1);
  pl.task_off.assign(in->task_off, in->task_off + pl.Q + 1);
  pl.task_q.assign((size_t)pl.n_task, 0);
  pl.unit_off.assign((size_t)pl.n_task + 1, 0);
  for (long long q = 0; q < pl.Q; ++q)
    for (long long t = pl.task_off[q]; t < pl.task_off[q + 1]; ++t) {
      if (in->task_db[t] < 0 || in->task_db[t] >= pl.n_db) {
        msg = "task " + std::to_string(t) + " names database image row " + std::to_string(in->task_db[t]) + " of " + std::to_string(pl.n_db);
        return 1;
      }
      pl.task_q[(size_t)t] = (int)q;
      pl.unit_off[(size_t)t + 1] = pl.unit_off[(size_t)t] + (pl.listed() ? 0 : pl.q_seg_off[q + 1] - pl.q_seg_off[q]);
    }
  if (pl.listed()) {
    pl.pair_off.assign(in->pair_off, in->pair_off + pl.n_task + 1);
    for (long long t = 0; t < pl.n_task; ++t) {
      const long long q = pl.task_q[(size_t)t], img = in->task_db[t];
      const long long nq = pl.q_seg_off[q + 1] - pl.q_seg_off[q], nd = pl.db_seg_off[img + 1] - pl.db_seg_off[img];
      for (long long p = pl.pair_off[t]; p < pl.pair_off[t + 1]; ++p) {
        const long long i = in->pairs2[2 * p], j = in->pairs2[2 * p + 1];
        if (i < 0 || i >= nq || j < 0 || j >= nd) {
          msg = "listed pair " + std::to_string(p) + " (" + std::to_string(i) + ", " + std::to_string(j) + ") is outside the " +
                std::to_string(nq) + " x " + std::to_string(nd) + " lines of task " + std::to_string(t);
          return 1;
        }
      }
    }
  }
  for (long long s = 0; s < pl.n_dbseg; ++s)
    if (in->db_track[s] < -1 || in->db_track[s] >= pl.T) {
      msg = "database segment " + std::to_string(s) + " has track id " + std::to_string(in->db_track[s]) + " (tracks: " + std::to_string(pl.T) + ")";
      return 1;
    }
  pl.n_units = pl.unit_off[(size_t)pl.n_task];
  if (pl.n_units > lim) {
    msg = "more than 2^31 - 1 (task, query line) units in one call (" + std::to_string(pl.n_units) + "): split the queries";
    return 1;
  }
  return 0;
}

// What grouping leaves: the rows of all queries in upstream's order and, per query, its keyed lines (slot q_seg_off[q] +
// p: the p-th line in key order, where its rows start within the query, how many).  The device path's scan and fill
// produce the same arrays.
struct Grouped {
  std::vector<long long> q_row0, q_total, kl_start, kl_cnt;
  std::vector<int> kl_line, rows2;
};

// seq[q]: the kept (query line, track id) pairs of query q in upstream's loop order, interleaved.  A line's key is its
// first appearance (the defaultdict's insertion); rows are sorted by (line key, sequence number), duplicates kept.
void group_rows(const Plan &pl, const std::vector<std::vector<int>> &seq, int n_threads, Grouped &g) {
  const long long Q = pl.Q;
  g.q_row0.assign((size_t)Q + 1, 0);
  g.q_total.assign(2 * (size_t)std::max<long long>(Q, 1), 0);
  g.kl_start.assign((size_t)std::max<long long>(pl.n_qseg, 1), 0);
  g.kl_cnt.assign((size_t)std::max<long long>(pl.n_qseg, 1), 0);
  g.kl_line.assign((size_t)std::max<long long>(pl.n_qseg, 1), 0);
  for (long long q = 0; q < Q; ++q) g.q_row0[(size_t)q + 1] = g.q_row0[(size_t)q] + (long long)seq[(size_t)q].size() / 2;
  g.rows2.assign(2 * (size_t)std::max<long long>(g.q_row0[(size_t)Q], 1), 0);
#pragma omp parallel for num_threads(n_threads) schedule(dynamic, 1)
  for (long long q = 0; q < Q; ++q) {
    const std::vector<int> &s = seq[(size_t)q];
    const long long s0 = pl.q_seg_off[(size_t)q], L = pl.q_seg_off[(size_t)q + 1] - s0, n = (long long)s.size() / 2;
    std::vector<long long> cnt((size_t)L, 0), next((size_t)L, 0);
    long long nk = 0;
    for (long long r = 0; r < n; ++r) {
      const int i = s[2 * (size_t)r];
      if (cnt[(size_t)i]++ == 0) g.kl_line[(size_t)(s0 + nk++)] = i;
    }
    long long run = 0;
    for (long long p = 0; p < nk; ++p) {
      const int i = g.kl_line[(size_t)(s0 + p)];
      g.kl_start[(size_t)(s0 + p)] = next[(size_t)i] = run;
      g.kl_cnt[(size_t)(s0 + p)] = cnt[(size_t)i];
      run += cnt[(size_t)i];
    }
    int *rows = g.rows2.data() + 2 * g.q_row0[(size_t)q];
    for (long long r = 0; r < n; ++r) {
      const long long o = next[(size_t)s[2 * (size_t)r]]++;
      rows[2 * o] = s[2 * (size_t)r];
      rows[2 * o + 1] = s[2 * (size_t)r + 1];
    }
    g.q_total[2 * (size_t)q] = n;
    g.q_total[2 * (size_t)q + 1] = nk;
  }
}

// the kept pairs of the listed modes in loop order, from their keep flags
void listed_sequences(const Plan &pl, const lt_l23_input *in, const unsigned char *keep, std::vector<std::vector<int>> &seq) {
  seq.assign((size_t)pl.Q, {});
  for (long long t = 0; t < pl.n_task; ++t) {
    std::vector<int> &s = seq[(size_t)pl.task_q[(size_t)t]];
    const long long j0 = pl.db_seg_off[(size_t)in->task_db[t]];
    for (long long p = pl.pair_off[(size_t)t]; p < pl.pair_off[(size_t)t + 1]; ++p)
      if (keep[p]) {
        s.push_back(in->pairs2[2 * p]);
        s.push_back(in->db_track[j0 + in->pairs2[2 * p + 1]]);
      }
  }
}

struct Result {
  std::vector<long long> q_off;
  std::vector<int> rows;
  std::vector<double> loss;
};

// without a filter the grouped rows are the result
void result_from_rows(const Plan &pl, const std::vector<long long> &q_row0, const int *rows2, Result &res) {
  res.q_off = q_row0;
  res.rows.assign(rows2, rows2 + 2 * q_row0[(size_t)pl.Q]);
  res.loss.assign((size_t)q_row0[(size_t)pl.Q], 0.0);
}

// with one: the winners, compacted per query from q_seg_off[q]
void result_from_winners(const Plan &pl, const long long *out_cnt, const int *out_rows2, const double *out_loss, Result &res) {
  res.q_off.assign((size_t)pl.Q + 1, 0);
  for (long long q = 0; q < pl.Q; ++q) res.q_off[(size_t)q + 1] = res.q_off[(size_t)q] + out_cnt[q];
  res.rows.resize(2 * (size_t)res.q_off[(size_t)pl.Q]);
  res.loss.resize((size_t)res.q_off[(size_t)pl.Q]);
  for (long long q = 0; q < pl.Q; ++q) {
    const long long s0 = pl.q_seg_off[(size_t)q], o = res.q_off[(size_t)q];
    std::copy(out_rows2 + 2 * s0, out_rows2 + 2 * (s0 + out_cnt[q]), res.rows.begin() + 2 * o);
    std::copy(out_loss + s0, out_loss + s0 + out_cnt[q], res.loss.begin() + o);
  }
}

// the whole definition on the host
void run_host(const Plan &pl, const lt_l23_input *in, int n_threads, Result &res) {
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  std::vector<Cam> db_cam((size_t)pl.n_db), q_cam((size_t)pl.Q);
  std::vector<L23DbSeg> db_rec((size_t)pl.n_dbseg);
  std::vector<double> F(9 * (size_t)pl.n_task);
  for (long long i = 0; i < pl.n_db; ++i) cam_build(in->db_cam11 + 11 * i, in->db_cam11 + 11 * i + 4, in->db_cam11 + 11 * i + 8, &db_cam[(size_t)i]);
  for (long long i = 0; i < pl.Q; ++i) cam_build(in->q_cam11 + 11 * i, in->q_cam11 + 11 * i + 4, in->q_cam11 + 11 * i + 8, &q_cam[(size_t)i]);
#pragma omp parallel for num_threads(nt) schedule(static)
  for (long long img = 0; img < pl.n_db; ++img)
    for (long long s = pl.db_seg_off[(size_t)img]; s < pl.db_seg_off[(size_t)img + 1]; ++s)
      l23_dbseg_build(db_cam[(size_t)img], in->db_seg4 + 4 * s, &db_rec[(size_t)s]);
  for (long long t = 0; t < pl.n_task; ++t) {
    PairRec p;
    pair_build(q_cam[(size_t)pl.task_q[(size_t)t]], db_cam[(size_t)in->task_db[t]], &p);
    std::copy(p.F, p.F + 9, F.begin() + 9 * t);
  }
  std::vector<std::vector<int>> seq((size_t)pl.Q);
  if (!pl.listed()) {
    // upstream's loop per query: tasks in retrieval order, query lines, database lines
#pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
    for (long long q = 0; q < pl.Q; ++q) {
      const long long s0 = pl.q_seg_off[(size_t)q], L = pl.q_seg_off[(size_t)q + 1] - s0;
      std::vector<int> &s = seq[(size_t)q];
      for (long long t = pl.task_off[(size_t)q]; t < pl.task_off[(size_t)q + 1]; ++t) {
        const long long img = in->task_db[t], j0 = pl.db_seg_off[(size_t)img], nd = pl.db_seg_off[(size_t)img + 1] - j0;
        for (long long i = 0; i < L; ++i)
          for (long long j = 0; j < nd; ++j)
            if (l23_iou_test(pl.cfg, in->q_seg4 + 4 * (s0 + i), db_rec[(size_t)(j0 + j)], F.data() + 9 * t) && in->db_track[j0 + j] != -1) {
              s.push_back((int)i);
              s.push_back(in->db_track[j0 + j]);
            }
      }
    }
  } else {
    std::vector<unsigned char> keep((size_t)pl.n_pairs, 0);
#pragma omp parallel for num_threads(nt) schedule(static)
    for (long long t = 0; t < pl.n_task; ++t) {
      const long long s0 = pl.q_seg_off[(size_t)pl.task_q[(size_t)t]], j0 = pl.db_seg_off[(size_t)in->task_db[t]];
      for (long long p = pl.pair_off[(size_t)t]; p < pl.pair_off[(size_t)t + 1]; ++p) {
        const long long i = s0 + in->pairs2[2 * p], j = j0 + in->pairs2[2 * p + 1];
        bool ok = true;
        if (pl.cfg.mode == kL23ListedFiltered) ok = l23_iou_test(pl.cfg, in->q_seg4 + 4 * i, db_rec[(size_t)j], F.data() + 9 * t);
        keep[(size_t)p] = ok && in->db_track[j] != -1;
      }
    }
    listed_sequences(pl, in, keep.data(), seq);
  }
  Grouped g;
  group_rows(pl, seq, nt, g);
  if (pl.cfg.filter == kL23NoFilter) {
    result_from_rows(pl, g.q_row0, g.rows2.data(), res);
    return;
  }
  // k_l23_filter and k_l23_compact
  std::vector<long long> out_cnt((size_t)pl.Q, 0);
  std::vector<int> out_rows2(2 * (size_t)std::max<long long>(pl.n_qseg, 1));
  std::vector<double> out_loss((size_t)std::max<long long>(pl.n_qseg, 1));
#pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
  for (long long q = 0; q < pl.Q; ++q) {
    const long long s0 = pl.q_seg_off[(size_t)q], nk = g.q_total[2 * (size_t)q + 1];
    long long run = 0;
    for (long long p = 0; p < nk; ++p) {
      const double *s4 = in->q_seg4 + 4 * (s0 + g.kl_line[(size_t)(s0 + p)]);
      const L2 ref{mk2(s4[0], s4[1]), mk2(s4[2], s4[3])};
      const long long start = g.q_row0[(size_t)q] + g.kl_start[(size_t)(s0 + p)], n = g.kl_cnt[(size_t)(s0 + p)];
      double best = kL23Inf;
      int best_t = INT_MAX;
      for (long long c = 0; c < n; ++c) {
        const int t = g.rows2[2 * (size_t)(start + c) + 1];
        const double loss = l23_cand_loss(pl.cfg, q_cam[(size_t)q], ref, in->track6 + 6 * (long long)t);
        if (l23_better(loss, t, best, best_t)) { best = loss; best_t = t; }
      }
      if (best < kL23Inf) {
        out_rows2[2 * (size_t)(s0 + run)] = g.kl_line[(size_t)(s0 + p)];
        out_rows2[2 * (size_t)(s0 + run) + 1] = best_t;
        out_loss[(size_t)(s0 + run)] = best;
        ++run;
      }
    }
    out_cnt[(size_t)q] = run;
  }
  result_from_winners(pl, out_cnt.data(), out_rows2.data(), out_loss.data(), res);
}

void copy_out(const Result &res, int64_t *q_off, int32_t *rows2, double *loss) {
  if (q_off) std::copy(res.q_off.begin(), res.q_off.end(), q_off);
  if (rows2) std::copy(res.rows.begin(), res.rows.end(), rows2);
  if (loss) std::copy(res.loss.begin(), res.loss.end(), loss);
}

thread_local HostError g_host_error;
thread_local Result g_host_result;

}  // namespace

extern "C" {

void lt_l23_config_default(lt_l23_config *c) {
  if (!c) return;
  c->mode = kL23AllPairs;
  c->filter = kL23NoFilter;
  c->IoU_threshold = 0.2;
  c->dist_thres = 10.0;  // functions.py:100-102
  c->sine_thres = 0.4;
  c->angle_scale = 1.0;
}

#ifndef LT_HOST_ONLY
int lt_l23_match(lt_ctx *ctx, const lt_l23_input *in, const lt_l23_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const double t0 = now_ms();
  std::string msg;
  Plan pl;
  if (make_plan(in, cfg, pl, msg)) return fail(ctx, LT_ERR_ARGUMENT, std::string(kWho) + ": " + msg);
  lt_host::L23State &s = ctx->l23;
  const long long Q = pl.Q;
  s.q_off.assign((size_t)Q + 1, 0);
  s.rows.clear();
  s.loss.clear();
  for (int k = 0; k < 8; ++k) s.timers[k] = 0.0;
  if (Q == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool filter = pl.cfg.filter != kL23NoFilter;
  const size_t one = 1;
  auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
    ENSURE(ctx, b, std::max(bytes, one * 8));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return LT_OK;
  };
  if (int rc = up(s.d_db_cam11, in->db_cam11, 88 * (size_t)pl.n_db)) return rc;
  if (int rc = up(s.d_q_cam11, in->q_cam11, 88 * (size_t)Q)) return rc;
  if (int rc = up(s.d_db_seg4, in->db_seg4, 32 * (size_t)pl.n_dbseg)) return rc;
  if (int rc = up(s.d_q_seg4, in->q_seg4, 32 * (size_t)pl.n_qseg)) return rc;
  if (int rc = up(s.d_track6, in->track6, filter ? 48 * (size_t)pl.T : 0)) return rc;
  if (int rc = up(s.d_db_track, in->db_track, 4 * (size_t)pl.n_dbseg)) return rc;
  if (int rc = up(s.d_task_db, in->task_db, 4 * (size_t)pl.n_task)) return rc;
  if (int rc = upload_vec(ctx, s.d_db_seg_off, pl.db_seg_off)) return rc;
  if (int rc = upload_vec(ctx, s.d_q_seg_off, pl.q_seg_off)) return rc;
  if (int rc = upload_vec(ctx, s.d_task_off, pl.task_off)) return rc;
  if (int rc = upload_vec(ctx, s.d_unit_off, pl.unit_off)) return rc;
  if (int rc = upload_vec(ctx, s.d_task_q, pl.task_q)) return rc;
  if (pl.listed()) {
    if (int rc = upload_vec(ctx, s.d_pair_off, pl.pair_off)) return rc;
    if (int rc = up(s.d_pairs, in->pairs2, 8 * (size_t)pl.n_pairs)) return rc;
    ENSURE(ctx, s.d_keep, std::max<size_t>((size_t)pl.n_pairs, 8));
  }
  const size_t nq1 = (size_t)std::max<long long>(pl.n_qseg, 1), nu1 = (size_t)std::max<long long>(pl.n_units, 1);
  ENSURE(ctx, s.d_db_cam, sizeof(Cam) * (size_t)std::max<long long>(pl.n_db, 1));
  ENSURE(ctx, s.d_q_cam, sizeof(Cam) * (size_t)Q);
  ENSURE(ctx, s.d_db_rec, sizeof(L23DbSeg) * (size_t)std::max<long long>(pl.n_dbseg, 1));
  ENSURE(ctx, s.d_task_F, 72 * (size_t)std::max<long long>(pl.n_task, 1));
  ENSURE(ctx, s.d_count, 4 * nu1);
  ENSURE(ctx, s.d_unit_pos, 4 * nu1);
  ENSURE(ctx, s.d_first, 4 * nq1);
  ENSURE(ctx, s.d_tot, 8 * nq1);
  ENSURE(ctx, s.d_kl_line, 4 * nq1);
  ENSURE(ctx, s.d_kl_start, 8 * nq1);
  ENSURE(ctx, s.d_kl_cnt, 8 * nq1);
  ENSURE(ctx, s.d_q_total, 16 * (size_t)Q);
  ENSURE(ctx, s.d_q_row0, 8 * ((size_t)Q + 1));
  if (filter) {
    ENSURE(ctx, s.d_win_track, 4 * nq1);
    ENSURE(ctx, s.d_win_loss, 8 * nq1);
    ENSURE(ctx, s.d_out_rows, 8 * nq1);
    ENSURE(ctx, s.d_out_loss, 8 * nq1);
    ENSURE(ctx, s.d_out_cnt, 8 * (size_t)Q);
  }
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  s.timers[0] = t1 - t0;

  L23Dev d{};
  d.cfg = pl.cfg;
  d.n_db = pl.n_db; d.n_query = Q; d.n_task = pl.n_task; d.n_dbseg = pl.n_dbseg; d.n_qseg = pl.n_qseg;
  d.n_units = pl.n_units; d.n_pairs = pl.n_pairs; d.n_tracks = pl.T;
  d.db_cam11 = s.d_db_cam11.as<double>(); d.q_cam11 = s.d_q_cam11.as<double>();
  d.db_seg4 = s.d_db_seg4.as<double>(); d.q_seg4 = s.d_q_seg4.as<double>(); d.track6 = s.d_track6.as<double>();
  d.db_seg_off = s.d_db_seg_off.as<long long>(); d.q_seg_off = s.d_q_seg_off.as<long long>();
  d.task_off = s.d_task_off.as<long long>(); d.unit_off = s.d_unit_off.as<long long>(); d.pair_off = s.d_pair_off.as<long long>();
  d.task_db = s.d_task_db.as<int>(); d.task_q = s.d_task_q.as<int>(); d.db_track = s.d_db_track.as<int>(); d.pairs2 = s.d_pairs.as<int>();
  d.db_cam = s.d_db_cam.as<Cam>(); d.q_cam = s.d_q_cam.as<Cam>(); d.db_rec = s.d_db_rec.as<L23DbSeg>(); d.task_F = s.d_task_F.as<double>();
  d.count = s.d_count.as<unsigned>(); d.unit_pos = s.d_unit_pos.as<unsigned>(); d.first = s.d_first.as<int>(); d.tot = s.d_tot.as<long long>();
  d.kl_line = s.d_kl_line.as<int>(); d.kl_start = s.d_kl_start.as<long long>(); d.kl_cnt = s.d_kl_cnt.as<long long>();
  d.q_total = s.d_q_total.as<long long>(); d.q_row0 = s.d_q_row0.as<long long>();
  d.keep = s.d_keep.as<unsigned char>();
  d.win_track = s.d_win_track.as<int>(); d.win_loss = s.d_win_loss.as<double>();
  d.out_rows2 = s.d_out_rows.as<int>(); d.out_loss = s.d_out_loss.as<double>(); d.out_cnt = s.d_out_cnt.as<long long>();

  Events<7> ev;  // build | count or flags | scan | (the readback) | fill | filter
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_l23_build(st, d);
  if (int rc = ev.record(ctx, 1)) return rc;
  std::vector<long long> q_row0((size_t)Q + 1, 0);
  Grouped g;
  const int *host_rows = nullptr;
  if (!pl.listed()) {
    launch_l23_count(st, d);
    if (int rc = ev.record(ctx, 2)) return rc;
    launch_l23_scan(st, d);
    if (int rc = ev.record(ctx, 3)) return rc;
    // the one readback between enqueue and download: the queries' totals size the output
    std::vector<long long> q_total;
    if (int rc = download(ctx, q_total, s.d_q_total.p, 2 * (size_t)Q)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    for (long long q = 0; q < Q; ++q) q_row0[(size_t)q + 1] = q_row0[(size_t)q] + q_total[2 * (size_t)q];
    const long long M = q_row0[(size_t)Q];
    if (M > INT_MAX) return fail(ctx, LT_ERR_ARGUMENT, std::string(kWho) + ": more than 2^31 - 1 rows in one call (" + std::to_string(M) + "): split the queries");
    ENSURE(ctx, s.d_rows, 8 * (size_t)std::max<long long>(M, 1));
    d.rows2 = s.d_rows.as<int>();
    d.rows_cap = M;
    if (int rc = upload_vec(ctx, s.d_q_row0, q_row0)) return rc;
    d.q_row0 = s.d_q_row0.as<long long>();
    if (int rc = ev.record(ctx, 4)) return rc;
    launch_l23_fill(st, d);
    if (int rc = ev.record(ctx, 5)) return rc;
  } else {
    launch_l23_listed(st, d);
    if (int rc = ev.record(ctx, 2)) return rc;
    std::vector<unsigned char> keep;
    if (int rc = download(ctx, keep, s.d_keep.p, (size_t)pl.n_pairs)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    std::vector<std::vector<int>> seq;
    listed_sequences(pl, in, keep.data(), seq);
    group_rows(pl, seq, omp_get_max_threads(), g);
    q_row0 = g.q_row0;
    host_rows = g.rows2.data();
    if (filter) {
      if (int rc = upload_vec(ctx, s.d_rows, g.rows2)) return rc;
      if (int rc = upload_vec(ctx, s.d_kl_line, g.kl_line)) return rc;
      if (int rc = upload_vec(ctx, s.d_kl_start, g.kl_start)) return rc;
      if (int rc = upload_vec(ctx, s.d_kl_cnt, g.kl_cnt)) return rc;
      if (int rc = upload_vec(ctx, s.d_q_total, g.q_total)) return rc;
      if (int rc = upload_vec(ctx, s.d_q_row0, g.q_row0)) return rc;
      d.rows2 = s.d_rows.as<int>();
      d.rows_cap = g.q_row0[(size_t)Q];
      d.kl_line = s.d_kl_line.as<int>(); d.kl_start = s.d_kl_start.as<long long>(); d.kl_cnt = s.d_kl_cnt.as<long long>();
      d.q_total = s.d_q_total.as<long long>(); d.q_row0 = s.d_q_row0.as<long long>();
    }
    if (int rc = ev.record(ctx, 5)) return rc;
  }
  if (filter) launch_l23_filter(st, d);
  if (int rc = ev.record(ctx, 6)) return rc;
  HIPCHK(ctx, hipGetLastError());
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  s.timers[1] = t2 - t1;
  s.timers[3] = ev.ms(0, 1); s.timers[4] = ev.ms(1, 2);
  if (!pl.listed()) { s.timers[5] = ev.ms(2, 3); s.timers[6] = ev.ms(4, 5); }
  s.timers[7] = ev.ms(5, 6);

  Result res;
  if (filter) {
    std::vector<long long> out_cnt;
    std::vector<int> out_rows2;
    std::vector<double> out_loss;
    if (int rc = download(ctx, out_cnt, s.d_out_cnt.p, (size_t)Q)) return rc;
    if (int rc = download(ctx, out_rows2, s.d_out_rows.p, 2 * (size_t)pl.n_qseg)) return rc;
    if (int rc = download(ctx, out_loss, s.d_out_loss.p, (size_t)pl.n_qseg)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    for (long long q = 0; q < Q; ++q)
      if (out_cnt[(size_t)q] < 0 || out_cnt[(size_t)q] > pl.q_seg_off[(size_t)q + 1] - pl.q_seg_off[(size_t)q])
        return fail(ctx, LT_ERR_STATE, std::string(kWho) + ": the compaction returned an impossible count");
    result_from_winners(pl, out_cnt.data(), out_rows2.data(), out_loss.data(), res);
  } else if (host_rows) {
    result_from_rows(pl, q_row0, host_rows, res);
  } else {
    std::vector<int> rows;
    if (int rc = download(ctx, rows, s.d_rows.p, 2 * (size_t)q_row0[(size_t)Q])) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    result_from_rows(pl, q_row0, rows.data(), res);
  }
  s.q_off.swap(res.q_off);
  s.rows.swap(res.rows);
  s.loss.swap(res.loss);
  s.timers[2] = now_ms() - t2;
  return LT_OK;
}

int64_t lt_l23_num(lt_ctx *ctx) { return ctx ? (int64_t)ctx->l23.loss.size() : 0; }

int lt_l23_get(lt_ctx *ctx, int64_t *q_off, int32_t *rows2, double *loss) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const lt_host::L23State &s = ctx->l23;
  if (q_off) std::copy(s.q_off.begin(), s.q_off.end(), q_off);
  if (rows2) std::copy(s.rows.begin(), s.rows.end(), rows2);
  if (loss) std::copy(s.loss.begin(), s.loss.end(), loss);
  return LT_OK;
}

int lt_l23_get_timers(lt_ctx *ctx, double out[8]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 8; ++k) out[k] = ctx->l23.timers[k];
  return LT_OK;
}
#endif  // LT_HOST_ONLY

const char *lt_fn_l23_host_error(void) { return g_host_error.c_str(); }

int lt_fn_l23_host(const lt_l23_input *in, const lt_l23_config *cfg, int host_threads, int64_t *n_rows) {
  std::string msg;
  Plan pl;
  g_host_result = Result();
  if (n_rows) *n_rows = 0;
  if (int rc = g_host_error.check(kWho, make_plan(in, cfg, pl, msg), msg)) return rc;
  run_host(pl, in, host_threads, g_host_result);
  if (n_rows) *n_rows = (int64_t)g_host_result.loss.size();
  return LT_OK;
}

int lt_fn_l23_host_get(int64_t *q_off, int32_t *rows2, double *loss) {
  copy_out(g_host_result, q_off, rows2, loss);
  return LT_OK;
}

}  // extern "C"
