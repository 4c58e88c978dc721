// dense_host_asan.cpp -- the host restatement of the dense-warp line matcher (lt_fn_match_dense_pair_host,
// lt_fn_match_dense_dists_host of lt_match_dense.cpp) under AddressSanitizer and UBSan, as a program of its own: the
// file is compiled into it with the sanitizers and without its device entry (LT_HOST_ONLY); nothing is loaded into
// Python and no device is touched.  `make -C limap_amd/csrc dense_asan` builds and runs it on two fixtures of
// tests/golden/match_dense (asan_*.bin: raw arrays written by make_match_dense_golden.py -- lines that leave the
// maps, maps whose aspect differs from the images', certainty holes, zero-length lines) and on the degenerate shapes:
// no lines on either side, 1 x 1 maps, NaN and infinity in a warp, every refusal.  Buffers are exactly as large as the
// sizes say: an overrun of one element is the sanitizer's to find.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

struct Pair {
  std::vector<float> l1, l2, w12, c12, w21, c21;
  int32_t s1[2], s2[2], d12[4], d21[4];
  lt_match_dense_config cfg;
  std::vector<int32_t> ref;
};

lt_match_dense_config config(int S, float seg, float pix, float th, int otm) {
  lt_match_dense_config c;
  c.n_samples = S;
  c.one_to_many = otm;
  c.segment_percentage_th = seg;
  c.pixel_th = pix;
  c.sample_thresh = th;
  c.on_device = c.want_scores = c.want_dirs = 0;
  return c;
}

template <class T>
bool read_n(std::FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

bool load(const std::string &path, Pair &p) {
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  int32_t h[16];
  float t[3];
  bool ok = std::fread(h, 4, 16, f) == 16 && std::fread(t, 4, 3, f) == 3;
  if (ok) {
    p.s1[0] = h[2]; p.s1[1] = h[3]; p.s2[0] = h[4]; p.s2[1] = h[5];
    p.d12[0] = p.d12[2] = h[6]; p.d12[1] = p.d12[3] = h[7];
    p.d21[0] = p.d21[2] = h[8]; p.d21[1] = p.d21[3] = h[9];
    p.cfg = config(h[10], t[0], t[1], t[2], 0);
    ok = read_n(f, p.l1, 4 * (size_t)h[0]) && read_n(f, p.l2, 4 * (size_t)h[1]) &&
         read_n(f, p.w12, 2 * (size_t)h[6] * h[7]) && read_n(f, p.c12, (size_t)h[6] * h[7]) &&
         read_n(f, p.w21, 2 * (size_t)h[8] * h[9]) && read_n(f, p.c21, (size_t)h[8] * h[9]) &&
         read_n(f, p.ref, 2 * (size_t)h[11]);
  }
  std::fclose(f);
  return ok;
}

struct Result {
  int rc;
  int64_t n;
  std::vector<int32_t> rows;
  std::vector<float> scores;
};

Result run(const Pair &p) {
  const int64_t n1 = (int64_t)p.l1.size() / 4, n2 = (int64_t)p.l2.size() / 4;
  Result r;
  r.rows.resize((size_t)(2 * n1 * n2));
  r.scores.resize((size_t)(n1 * n2));
  r.n = -1;
  r.rc = lt_fn_match_dense_pair_host(p.l1.data(), n1, p.s1, p.l2.data(), n2, p.s2, p.w12.data(), p.c12.data(), p.d12,
                                     p.w21.data(), p.c21.data(), p.d21, &p.cfg, r.rows.data(), r.scores.data(), &r.n);
  std::vector<float> a((size_t)(n1 * n2)), b(a), c(a), d(a), e(a);
  const int rc2 = lt_fn_match_dense_dists_host(p.l1.data(), n1, p.s1, p.l2.data(), n2, p.s2, p.w12.data(), p.c12.data(),
                                               p.d12, p.w21.data(), p.c21.data(), p.d21, &p.cfg, a.data(), b.data(),
                                               c.data(), d.data(), e.data());
  EXPECT(rc2 == r.rc);
  return r;
}

Pair tiny(int n1, int n2, int hw, int ww, float value) {
  Pair p;
  for (int k = 0; k < n1; ++k) { p.l1.push_back(3.f + k); p.l1.push_back(4.f); p.l1.push_back(40.f); p.l1.push_back(30.f + k); }
  for (int k = 0; k < n2; ++k) { p.l2.push_back(5.f); p.l2.push_back(6.f + k); p.l2.push_back(44.f + k); p.l2.push_back(28.f); }
  p.s1[0] = 48; p.s1[1] = 64; p.s2[0] = 40; p.s2[1] = 56;
  p.d12[0] = p.d12[2] = p.d21[0] = p.d21[2] = hw;
  p.d12[1] = p.d12[3] = p.d21[1] = p.d21[3] = ww;
  p.w12.assign((size_t)(2 * hw * ww), value);
  p.w21 = p.w12;
  p.c12.assign((size_t)(hw * ww), 0.9f);
  p.c21 = p.c12;
  p.cfg = config(21, 0.2f, 10.0f, 0.5f, 0);
  return p;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : "tests/golden/match_dense";
  for (const char *name : {"asan_aspect_holes_33_37.bin", "asan_zero_length_12_12.bin"}) {
    Pair p;
    const bool ok = load(dir + "/" + name, p);
    EXPECT(ok);
    if (!ok) continue;
    Result r = run(p);
    EXPECT(r.rc == 0);
    // upstream's rows and the restatement's differ on undecided entries only: here the counts are reported, the
    // comparison under the decided rule is tests/test_match_dense_host.py's
    std::printf("%s: %lld rows (upstream %zu)\n", name, (long long)r.n, p.ref.size() / 2);
    for (int64_t k = 0; k < r.n; ++k) EXPECT(r.scores[(size_t)k] <= p.cfg.pixel_th);
    p.cfg.one_to_many = 1;
    Result m = run(p);
    EXPECT(m.rc == 0 && m.n >= r.n);
    for (int S : {2, 63, 64}) {
      p.cfg.n_samples = S;
      EXPECT(run(p).rc == 0);
    }
  }
  // degenerate shapes
  for (int n1 : {0, 1, 17})
    for (int n2 : {0, 1, 17})
      for (int hw : {1, 5}) EXPECT(run(tiny(n1, n2, hw, hw == 1 ? 1 : 3, 0.25f)).rc == 0);
  for (float bad : {NAN, INFINITY, -INFINITY, 3.0e38f}) {
    Result r = run(tiny(5, 4, 3, 2, bad));
    EXPECT(r.rc == 0 && r.n == 0);
  }
  {
    Pair p = tiny(3, 3, 2, 2, 0.0f);  // a zero-length line on either side
    p.l1[2] = p.l1[0]; p.l1[3] = p.l1[1];
    p.l2[6] = p.l2[4]; p.l2[7] = p.l2[5];
    EXPECT(run(p).rc == 0);
  }
  // ---- refusals ----
  {
    Pair p = tiny(2, 2, 2, 2, 0.0f);
    p.cfg.n_samples = 1;
    EXPECT(run(p).rc != 0);
    p.cfg.n_samples = 65;
    EXPECT(run(p).rc != 0);
    p.cfg.n_samples = 21;
    p.d12[0] = 0;
    EXPECT(run(p).rc != 0);
    p.d12[0] = 2;
    p.d21[3] = 3;
    EXPECT(run(p).rc != 0);
    p.d21[3] = 2;
    p.s1[1] = 0;
    EXPECT(run(p).rc != 0);
    p.s1[1] = 64;
    p.cfg.pixel_th = NAN;
    EXPECT(run(p).rc != 0);
    p.cfg.pixel_th = 10.0f;
    EXPECT(run(p).rc == 0);
  }
  return finish("dense_host_asan");
}
