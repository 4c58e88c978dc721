// l23_host_asan.cpp -- the host twin of limap_amd.localization's 2D-3D line matching (lt_fn_l23_host of lt_l23.cpp) under
// AddressSanitizer and UBSan, as a program of its own: lt_l23.cpp is compiled into it with LT_HOST_ONLY and the
// sanitizers; nothing is loaded into Python and no device is touched.  `make -C limap_amd/csrc l23_asan` builds and runs
// it (tests/test_l23_host.py does that).
// The cases are the edge shapes: database images with 0, 1, 63, 64, 65 and 130 lines, queries with 5, 0 and 1 lines and
// 3, 1 and 0 tasks (one image twice), segments of zero length, a query at a database pose, the three modes, the four
// filter kinds, empty input, and every refusal.
#include "host_asan.h"

#include <algorithm>
#include <cstring>

namespace {

struct Scene {
  std::vector<double> db_cam, db_seg, q_cam, q_seg, track;
  std::vector<int64_t> db_off{0}, q_off{0}, task_off{0}, pair_off{0};
  std::vector<int32_t> db_track, task_db, pairs;
  lt_l23_input in() const {
    lt_l23_input i;
    std::memset(&i, 0, sizeof i);
    i.n_db = (int64_t)db_off.size() - 1; i.db_cam11 = db_cam.data(); i.db_seg_off = db_off.data(); i.db_seg4 = db_seg.data();
    i.db_track = db_track.data();
    i.n_query = (int64_t)q_off.size() - 1; i.q_cam11 = q_cam.data(); i.q_seg_off = q_off.data(); i.q_seg4 = q_seg.data();
    i.task_off = task_off.data(); i.task_db = task_db.data();
    i.pair_off = pair_off.size() > 1 ? pair_off.data() : nullptr; i.pairs2 = pairs.data();
    i.n_tracks = (int64_t)track.size() / 6; i.track6 = track.data();
    return i;
  }
};

void add_cam(std::vector<double> &v, double a, double tx) {
  const double c[11] = {600, 590, 400, 300, std::cos(a), 0.0, std::sin(a), 0.0, tx, 0.01, 0.1};
  v.insert(v.end(), c, c + 11);
}

Scene make_scene() {
  Scene s;
  unsigned st = 7u;
  const int T = 130;
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < 2; ++k) {
      s.track.push_back(2.0 * jitter(st));
      s.track.push_back(1.5 * jitter(st));
      s.track.push_back(6.0 + jitter(st));
    }
  const int n_lines[6] = {0, 1, 63, 64, 65, 130};
  for (int d = 0; d < 6; ++d) {
    add_cam(s.db_cam, 0.01 * d, 0.3 * d - 0.7);
    for (int j = 0; j < n_lines[d]; ++j) {
      const double x = 400 + 300 * jitter(st), y = 300 + 200 * jitter(st);
      const bool zero = d == 5 && j == 9;
      const double seg[4] = {x, y, zero ? x : x + 80 * jitter(st), zero ? y : y + 80 * jitter(st)};
      s.db_seg.insert(s.db_seg.end(), seg, seg + 4);
      s.db_track.push_back(j % 3 == 2 ? -1 : (j * 7 + d) % T);
    }
    s.db_off.push_back((int64_t)s.db_seg.size() / 4);
  }
  const int q_lines[3] = {5, 0, 1};
  for (int q = 0; q < 3; ++q) {
    if (q == 2) s.q_cam.insert(s.q_cam.end(), s.db_cam.begin() + 44, s.db_cam.begin() + 55);  // the pose of image 4
    else add_cam(s.q_cam, 0.02, 0.05 * q);
    for (int i = 0; i < q_lines[q]; ++i) {
      const double x = 400 + 300 * jitter(st), y = 300 + 200 * jitter(st);
      const bool zero = q == 0 && i == 3;
      const double seg[4] = {x, y, zero ? x : x + 90 * jitter(st), zero ? y : y + 90 * jitter(st)};
      s.q_seg.insert(s.q_seg.end(), seg, seg + 4);
    }
    s.q_off.push_back((int64_t)s.q_seg.size() / 4);
  }
  const int32_t tasks[] = {5, 0, 5, 2, 4, 3, 1};  // query 0: 5, 0, 5; query 1: 2; query 2: 4, 3, 1
  s.task_db.assign(tasks, tasks + 7);
  s.task_off = {0, 3, 4, 7};
  return s;
}

void add_pairs(Scene &s) {
  unsigned st = 11u;
  s.pair_off = {0};
  s.pairs.clear();
  for (size_t q = 0; q + 1 < s.task_off.size(); ++q)
    for (int64_t t = s.task_off[q]; t < s.task_off[q + 1]; ++t) {
      const int64_t nq = s.q_off[q + 1] - s.q_off[q], nd = s.db_off[(size_t)s.task_db[(size_t)t] + 1] - s.db_off[(size_t)s.task_db[(size_t)t]];
      for (int k = 0; k < (nq && nd ? 70 : 0); ++k) {
        s.pairs.push_back((int32_t)((jitter(st) + 1.0) * 0.5 * (double)nq) % (int32_t)nq);
        s.pairs.push_back((int32_t)((jitter(st) + 1.0) * 0.5 * (double)nd) % (int32_t)nd);
      }
      s.pair_off.push_back((int64_t)s.pairs.size() / 2);
    }
  if (s.pairs.empty()) s.pairs.push_back(0);
}

struct Out {
  int rc = 0;
  std::vector<int64_t> off;
  std::vector<int32_t> rows;
  std::vector<double> loss;
};

Out run(const Scene &s, int mode, int filter, int threads, double thr = 0.2) {
  lt_l23_config c;
  lt_l23_config_default(&c);
  c.mode = mode; c.filter = filter; c.IoU_threshold = thr;
  const lt_l23_input in = s.in();
  Out o;
  int64_t n = -1;
  o.rc = lt_fn_l23_host(&in, &c, threads, &n);
  if (o.rc != 0) return o;
  // exactly as large as the counts say: an overrun of one element is the sanitizer's to find
  o.off.resize((size_t)in.n_query + 1);
  o.rows.resize(2 * (size_t)n);
  o.loss.resize((size_t)n);
  lt_fn_l23_host_get(o.off.data(), o.rows.data(), o.loss.data());
  return o;
}

void check_shape(const Scene &s, const Out &o, int filter) {
  EXPECT(o.rc == 0);
  if (o.rc != 0) return;
  EXPECT(o.off.front() == 0 && o.off.back() == (int64_t)o.loss.size());
  for (size_t q = 0; q + 1 < o.off.size(); ++q) {
    EXPECT(o.off[q] <= o.off[q + 1]);
    const int64_t nq = s.q_off[q + 1] - s.q_off[q];
    std::vector<int> seen((size_t)nq, 0);
    for (int64_t r = o.off[q]; r < o.off[q + 1]; ++r) {
      const int32_t i = o.rows[2 * (size_t)r], t = o.rows[2 * (size_t)r + 1];
      EXPECT(i >= 0 && i < nq && t >= 0 && t < (int32_t)(s.track.size() / 6));
      if (i >= 0 && i < nq) seen[(size_t)i] += 1;
      if (filter) EXPECT(std::isfinite(o.loss[(size_t)r]));
    }
    if (filter)
      for (int v : seen) EXPECT(v <= 1);
  }
}

bool refused(const Scene &s, int mode, int filter, const char *what) {
  const Out o = run(s, mode, filter, 1);
  return o.rc == LT_ERR_ARGUMENT && has(lt_fn_l23_host_error, what) && has(lt_fn_l23_host_error, "limap_amd.localization: ");
}

}  // namespace

int main() {
  Scene s = make_scene();
  Scene listed = s;
  add_pairs(listed);
  long long rows_seen = 0;
  for (int mode = 0; mode < 3; ++mode)
    for (int filter = 0; filter < 4; ++filter) {
      const Scene &sc = mode ? listed : s;
      const Out a = run(sc, mode, filter, 1), b = run(sc, mode, filter, 3);
      check_shape(sc, a, filter);
      EXPECT(a.off == b.off && a.rows == b.rows && a.loss == b.loss);
      rows_seen += (long long)a.loss.size();
    }
  EXPECT(rows_seen > 0);
  // query 1 has no lines, between two that have some
  const Out plain = run(s, 0, 0, 2);
  EXPECT(plain.rc == 0 && plain.off.size() == 4 && plain.off[1] == plain.off[2] && plain.off[1] > 0);
  // every pair failing: no rows
  const Out none = run(s, 0, 0, 2, 2.0);
  EXPECT(none.rc == 0 && none.loss.empty() && none.off.back() == 0);
  // no queries; no database
  Scene empty;
  EXPECT(run(empty, 0, 0, 1).rc == 0);
  Scene nodb = s;
  nodb.task_off = {0, 0, 0, 0};
  const Out nd = run(nodb, 0, 1, 1);
  EXPECT(nd.rc == 0 && nd.loss.empty());

  // refusals
  { Scene b = s; b.db_cam[13] = NAN; EXPECT(refused(b, 0, 0, "non-finite camera of database image 1")); }
  { Scene b = s; b.q_seg[4 * 5 + 2] = INFINITY; EXPECT(refused(b, 0, 0, "non-finite query segment 5")); }
  { Scene b = s; b.db_seg[4 * 100] = NAN; EXPECT(refused(b, 0, 0, "non-finite database segment 100")); }
  { Scene b = s; b.track[6 * 3 + 1] = NAN; EXPECT(refused(b, 0, 2, "non-finite track 3")); EXPECT(run(b, 0, 0, 1).rc == 0); }
  { Scene b = s; b.db_off[3] = 0; EXPECT(refused(b, 0, 0, "database segment offsets decrease")); }
  { Scene b = s; b.task_off[1] = 9; EXPECT(refused(b, 0, 0, "task offsets decrease")); }
  { Scene b = s; b.task_db[6] = 6; EXPECT(refused(b, 0, 0, "task 6 names database image row 6")); }
  { Scene b = listed; b.pairs[1] = 130; EXPECT(refused(b, 1, 0, "listed pair 0")); }
  { Scene b = listed; b.pairs[0] = -1; EXPECT(refused(b, 2, 0, "listed pair 0")); }
  { Scene b = s; b.db_track[0] = 130; EXPECT(refused(b, 0, 0, "has track id 130")); }
  { Scene b = s; b.db_track[5] = -2; EXPECT(refused(b, 0, 0, "has track id -2")); }
  EXPECT(refused(s, 3, 0, "unknown mode 3"));
  EXPECT(refused(s, 0, 4, "unknown filter kind 4"));
  EXPECT(refused(s, 1, 0, "null pair offsets"));
  // a refusal leaves no result behind; a good call clears the error
  int64_t off0[4] = {-1, -1, -1, -1};
  (void)refused(s, 3, 0, "unknown");
  lt_fn_l23_host_get(off0, nullptr, nullptr);
  EXPECT(off0[0] == -1);
  EXPECT(run(s, 0, 0, 1).rc == 0 && std::string(lt_fn_l23_host_error()).empty());
  return finish("l23_host_asan");
}
