// refine_feature_host_asan.cpp -- the host twin of the feature-consistency term (lt_fn_refine_host_feature,
// lt_fn_refine_eval_feature and the sample builder of lt_refine.cpp) under AddressSanitizer and UBSan, as a program of
// its own: lt_refine.cpp is compiled into it with LT_HOST_ONLY and the sanitizers; nothing is loaded into Python
// and no device is touched.  `make -C limap_amd/csrc refine_feature_asan` builds and runs it.
// The cases are the edge scenes of tests/test_refine_feature_host.py on four unrotated cameras beside a line along x: grids
// of 1x1, 3x4 and 6x40 texels that the intersections leave on every side (the clamp), both texel types, a rotated
// transform, supports beside the projection by just under and just over 0.3 px, points with one support, all supports
// of a point in one image, a sample line parallel to the projection (termination code 6), and every refusal.  The texel
// buffers are exactly h * w * 128 texels: a read past a grid is the sanitizer's to find.
#include "host_asan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

bool has(const char *what) { return host_asan::has(lt_fn_refine_host_error, what); }

const int32_t kIds[4] = {3, 5, 6, 9};
const double kK[16] = {64, 64, 32, 24, 64, 64, 32, 24, 64, 64, 32, 24, 64, 64, 32, 24};
const double kQ[16] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
const double kT[12] = {0, 0, 0, 0.25, 0.125, 0, -0.25, -0.25, 0, 0.5, 0.0625, 0};  // (off the x axis: no epipolar line is the projection)
double row_of(int c) { return 24.0 + 16.0 * kT[3 * c + 1]; }
const double kLine[6] = {-1.0, 0.0, 4.0, 1.0, 0.0, 4.0};

struct Scene {
  std::vector<int32_t> img;
  std::vector<double> l2d, l3d;
  std::vector<std::vector<unsigned char>> tex;  // one buffer per grid, exactly its size
  std::vector<lt_refine_grid> grids;
};

// the projection of the line into camera c: the row y = row_of(c) + dy from x0 to x1
void support(Scene &s, int c, double lo, double hi, double dy) {
  const double xa = 64.0 * (-1.0 + kT[3 * c]) / 4.0 + 32.0, xb = 64.0 * (1.0 + kT[3 * c]) / 4.0 + 32.0;
  s.img.push_back(kIds[c]);
  const double seg[4] = {xa + lo * (xb - xa), row_of(c) + dy, xa + hi * (xb - xa), row_of(c) + dy};
  s.l2d.insert(s.l2d.end(), seg, seg + 4);
  s.l3d.insert(s.l3d.end(), kLine, kLine + 6);
}

void grid(Scene &s, int h, int w, int type, bool rotated) {
  const size_t px = type == LT_TEXEL_F32 ? 4 : 2;
  s.tex.emplace_back((size_t)h * w * 128 * px);
  std::vector<unsigned char> &b = s.tex.back();
  for (size_t k = 0; k < b.size() / px; ++k) {
    if (type == LT_TEXEL_F32) {
      const float v = (float)((k * 37 % 101) / 101.0);
      std::memcpy(&b[4 * k], &v, 4);
    } else {
      const uint16_t v = (uint16_t)(0x3000 + (k * 37 % 1024));  // finite halves in [0.125, 0.25)
      std::memcpy(&b[2 * k], &v, 2);
    }
  }
  lt_refine_grid g;
  std::memset(&g, 0, sizeof(g));
  g.h = h; g.w = w;
  if (rotated) { g.R[0] = 0.0; g.R[1] = -1.0; g.R[2] = 1.0; g.R[3] = 0.0; g.tvec[0] = 20.0; g.tvec[1] = 26.0; }
  else { g.R[0] = 1.0; g.R[3] = 1.0; g.tvec[0] = 18.0; g.tvec[1] = 22.0; }
  s.grids.push_back(g);
}

void bind_grids(Scene &s) {
  for (size_t k = 0; k < s.grids.size(); ++k) s.grids[k].data = s.tex[k].data();
}

struct Out {
  double p[6], seg[6], cost[2];
  int32_t it, code;
};

int run(const Scene &s, int type, int n_samples, int threads, Out *o, int use_geometric = 1, int n_grids = -1) {
  lt_refine_config cfg;
  lt_refine_config_default(&cfg);
  cfg.max_num_iterations = 8;
  cfg.num_outliers_aggregator = 0;
  lt_refine_terms terms;
  lt_refine_terms_default(&terms);
  terms.use_geometric = use_geometric;
  lt_refine_feature feat;
  lt_refine_feature_default(&feat);
  feat.n_samples_feature = n_samples;
  feat.texel_type = type;
  const int64_t off[2] = {0, (int64_t)s.img.size()};
  return lt_fn_refine_host_feature(4, kIds, kK, kQ, kT, 1, kLine, off, s.img.data(), s.l2d.data(), s.l3d.data(), &cfg, &terms,
                                   nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &feat,
                                   n_grids < 0 ? (int64_t)s.grids.size() : n_grids, s.grids.data(), threads, o->p, o->seg, o->cost,
                                   &o->it, &o->code);
}

// the kept samples and the blocks of the scene at its initial line
int eval(const Scene &s, int type, int n_samples, int *n_kept, int *n_blocks, std::vector<int32_t> *failed) {
  lt_refine_terms terms;
  lt_refine_terms_default(&terms);
  lt_refine_feature feat;
  lt_refine_feature_default(&feat);
  feat.n_samples_feature = n_samples;
  feat.texel_type = type;
  const int cap_b = n_samples * 3;
  std::vector<int32_t> ref((size_t)n_samples), ntgt((size_t)n_samples), tg((size_t)cap_b);
  std::vector<double> line(3 * (size_t)n_samples), res(128 * (size_t)cap_b);
  failed->assign((size_t)cap_b, 0);
  int32_t nk = 0, nb = 0;
  double cost, g[4], H[16];
  const int rc = lt_fn_refine_eval_feature(4, kIds, kK, kQ, kT, kLine, (int64_t)s.img.size(), s.img.data(), s.l2d.data(), 10.0,
                                           &terms, &feat, (int64_t)s.grids.size(), s.grids.data(), nullptr, n_samples, cap_b, &nk,
                                           ref.data(), line.data(), ntgt.data(), tg.data(), &nb, res.data(), failed->data(), &cost,
                                           g, H);
  *n_kept = nk;
  *n_blocks = nb;
  return rc;
}

Scene plain(int type, double dy, int h, int w, bool rotated) {
  Scene s;
  for (int c = 0; c < 4; ++c) {
    support(s, c, 0.0, 1.0, dy);
    grid(s, h, w, type, rotated);
  }
  bind_grids(s);
  return s;
}

}  // namespace

int main() {
  Out o;
  int nk, nb;
  std::vector<int32_t> failed;
  for (int type : {LT_TEXEL_F16, LT_TEXEL_F32})
    for (int threads : {1, 4}) {
      for (bool rot : {false, true}) {
        Scene a = plain(type, 0.0, 6, 40, rot), b = plain(type, 0.0, 3, 4, rot), c = plain(type, 0.0, 1, 1, rot);
        EXPECT(run(a, type, 8, threads, &o) == 0 && std::isfinite(o.cost[0]) && o.cost[1] <= o.cost[0]);
        EXPECT(run(b, type, 8, threads, &o) == 0 && std::isfinite(o.cost[0]));
        EXPECT(run(c, type, 2, threads, &o) == 0 && std::isfinite(o.cost[0]));
        EXPECT(run(a, type, 8, threads, &o, 0) == 0);  // the feature term alone
        EXPECT(eval(a, type, 8, &nk, &nb, &failed) == 0 && nk == 6 && nb == 18);
      }
      // beside the projection by just under and just over 0.3 px
      Scene under = plain(type, 0.3 - 1e-9, 3, 4, false), over = plain(type, 0.3 + 1e-9, 3, 4, false);
      EXPECT(eval(under, type, 8, &nk, &nb, &failed) == 0 && nk == 6);
      EXPECT(eval(over, type, 8, &nk, &nb, &failed) == 0 && nk == 0 && nb == 0);
      EXPECT(run(over, type, 8, threads, &o) == 0 && o.code != 6);
    }
  {  // the first half has one support, then all supports of the points in one image, then three images
    Scene s;
    support(s, 0, 0.0, 0.3, 0.0);
    support(s, 1, 0.35, 0.6, 0.0);
    support(s, 1, 0.35, 0.62, 0.0);
    for (int c = 1; c < 4; ++c) support(s, c, 0.65, 1.0, 0.0);
    for (int c = 0; c < 4; ++c) grid(s, 3, 4, LT_TEXEL_F16, false);
    bind_grids(s);
    EXPECT(eval(s, LT_TEXEL_F16, 12, &nk, &nb, &failed) == 0 && nk > 0 && nk < 12 && nb > 0 && nb < 2 * nk);
    EXPECT(run(s, LT_TEXEL_F16, 12, 2, &o) == 0);
  }
  {  // a vertical support, the longest good one of the one point the others cover: the sample line is parallel to the projection
    Scene s;
    const double x3 = -1.0 + 3.0 * (2.0 / 7.0);
    for (int c = 0; c < 4; ++c) {
      const double x = 64.0 * (x3 + kT[3 * c]) / (4.0 + 1e-12) + 32.0;
      s.img.push_back(kIds[c]);
      const double v[4] = {x, 23.75, x, 24.25}, hz[4] = {x - 0.2, row_of(c), x + 0.2, row_of(c)};
      s.l2d.insert(s.l2d.end(), c == 0 ? v : hz, (c == 0 ? v : hz) + 4);
      s.l3d.insert(s.l3d.end(), kLine, kLine + 6);
      grid(s, 3, 4, LT_TEXEL_F16, false);
    }
    bind_grids(s);
    EXPECT(eval(s, LT_TEXEL_F16, 8, &nk, &nb, &failed) == 0 && nk == 1 && nb == 3 && failed[0] && failed[1] && failed[2]);
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) == 0 && o.code == 6 && o.it == 0 && std::isinf(o.cost[0]));
  }
  // ---- refusals ----
  {
    Scene s = plain(LT_TEXEL_F16, 0.0, 3, 4, false);
    EXPECT(run(s, LT_TEXEL_F16, 1, 1, &o) != 0 && has("n_samples_feature"));
    EXPECT(run(s, 7, 8, 1, &o) != 0 && has("texel type"));
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o, 1, 3) != 0 && has("fewer grids"));
    s.grids.push_back(s.grids[0]);
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) != 0 && has("more grids"));
    s.grids.pop_back();
    s.grids[1].data = s.tex[1].data() + 2;
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) != 0 && has("aligned"));
    s.grids[1].data = s.tex[1].data();
    s.grids[2].on_device = 1;
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) != 0 && has("on the device"));
    s.grids[2].on_device = 0;
    s.grids[3].h = 0;
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) != 0 && has("is empty"));
    s.grids[3].h = 3;
    s.grids[0].R[2] = NAN;
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) != 0 && has("transform"));
    s.grids[0].R[2] = 0.0;
    s.l2d[4] = s.l2d[6]; s.l2d[5] = s.l2d[7];  // a support of zero length is no support and no reference
    EXPECT(run(s, LT_TEXEL_F16, 8, 1, &o) == 0);
    lt_refine_feature feat;
    lt_refine_feature_default(&feat);
    EXPECT(feat.use_feature == 1 && feat.n_samples_feature == 100 && feat.fconsis_multiplier == 1.0 && feat.channels == 128);
  }
  return finish("refine_feature_host_asan");
}
