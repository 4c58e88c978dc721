// merge_ref_driver.cpp -- C entry points over the reference's own merging code, for make_merge_golden.py.
//
// Linked against the objects `make -C oracle ref` compiles from the reference's sources (oracle/_ref/obj/**/*.o) and
// built with the stand-in headers of oracle/ref_shim.  mrg_run performs what limap.merging.merging and the steps after
// it in runners/line_fitnmerge.py:226-258 do, with the reference's own functions:
//   SetUncertaintySegs3d, MergeToLineTracks (+ ComputeLineTrackLabelsGreedy for the labels of its graph),
//   FilterSupportingLines (num_outliers 0), RemergeLineTracks (num_outliers 0, to its fixed point like merging.py:24-42),
//   FilterSupportingLines (num_outliers 0).
#include "limap/base/graph.h"
#include "limap/base/image_collection.h"
#include "limap/base/line_linker.h"
#include "limap/base/linebase.h"
#include "limap/base/linetrack.h"
#include "limap/merging/merging.h"
#include "limap/merging/merging_utils.h"

#include <omp.h>

#include <chrono>
#include <cstdint>
#include <map>
#include <vector>

using namespace limap;

namespace {
struct Result {
  std::vector<int> node_img, node_line, e1, e2, labels;
  std::vector<double> sim;
  std::vector<LineTrack> stages[4];  // merge, filter, remerge, filter
  double merge_ms = 0.0;
};

void set2d(LineLinker2dConfig &c, const double *v) {
  c.score_th = v[0]; c.th_angle = v[1]; c.th_overlap = v[2]; c.th_smartoverlap = v[3]; c.th_smartangle = v[4];
  c.th_perp = v[5]; c.th_innerseg = v[6];
  c.use_angle = v[7] != 0; c.use_overlap = v[8] != 0; c.use_smartangle = v[9] != 0; c.use_perp = v[10] != 0;
  c.use_innerseg = v[11] != 0;
}
void set3d(LineLinker3dConfig &c, const double *v) {
  c.score_th = v[0]; c.th_angle = v[1]; c.th_overlap = v[2]; c.th_smartoverlap = v[3]; c.th_smartangle = v[4];
  c.th_perp = v[5]; c.th_innerseg = v[6]; c.th_scaleinv = v[7];
  c.use_angle = v[8] != 0; c.use_overlap = v[9] != 0; c.use_smartangle = v[10] != 0; c.use_perp = v[11] != 0;
  c.use_innerseg = v[12] != 0; c.use_scaleinv = v[13] != 0;
}
}  // namespace

extern "C" {

// l2[12], l3[14], rm3[14]: config fields in the order of set2d / set3d; returns a handle for the getters
void *mrg_run(int n_img, const int32_t *ids, const double *kvec, const double *qvec, const double *tvec,
              const int64_t *seg_off, const double *segs2, const double *segs3, const int64_t *nb_off,
              const int32_t *nb, const double *l2, const double *l3, double var2d, double th_angular2d,
              double th_perp2d, const double *rm3, int n_threads) {
  if (n_threads > 0) omp_set_num_threads(n_threads);
  std::map<int, Camera> cameras;
  std::map<int, CameraImage> images;
  std::map<int, Eigen::MatrixXd> arr2;
  std::map<int, std::vector<Eigen::MatrixXd>> arr3;
  std::map<int, std::vector<int>> neighbors;
  for (int i = 0; i < n_img; ++i) {
    const int id = ids[i];
    cameras.insert(std::make_pair(id, Camera(1, std::vector<double>{kvec[4 * i], kvec[4 * i + 1], kvec[4 * i + 2],
                                                                   kvec[4 * i + 3]}, id)));
    CameraPose pose(V4D(qvec[4 * i], qvec[4 * i + 1], qvec[4 * i + 2], qvec[4 * i + 3]),
                    V3D(tvec[3 * i], tvec[3 * i + 1], tvec[3 * i + 2]));
    images.insert(std::make_pair(id, CameraImage(id, pose)));
    const int64_t m = seg_off[i + 1] - seg_off[i];
    Eigen::MatrixXd a(m, 4);
    std::vector<Eigen::MatrixXd> b;
    for (int64_t l = 0; l < m; ++l) {
      for (int k = 0; k < 4; ++k) a(l, k) = segs2[4 * (seg_off[i] + l) + k];
      Eigen::MatrixXd s(2, 3);
      for (int r = 0; r < 2; ++r)
        for (int k = 0; k < 3; ++k) s(r, k) = segs3[6 * (seg_off[i] + l) + 3 * r + k];
      b.push_back(s);
    }
    arr2[id] = a;
    arr3[id] = b;
    neighbors[id] = std::vector<int>(nb + nb_off[i], nb + nb_off[i + 1]);
  }
  ImageCollection imagecols(cameras, images);
  // merging.py:6-21
  std::map<int, std::vector<Line2d>> all_lines_2d;
  std::map<int, std::vector<Line3d>> all_lines_3d;
  for (int id : imagecols.get_img_ids()) {
    all_lines_2d[id] = GetLine2dVectorFromArray(arr2[id]);
    all_lines_3d[id] = merging::SetUncertaintySegs3d(GetLine3dVectorFromArray(arr3[id]), imagecols.camview(id), var2d);
  }
  LineLinker2dConfig c2;
  LineLinker3dConfig c3, cr;
  set2d(c2, l2);
  set3d(c3, l3);
  set3d(cr, rm3);
  LineLinker linker(c2, c3);
  Result *res = new Result();
  Graph graph;
  std::vector<LineTrack> tracks;
  const auto t0 = std::chrono::steady_clock::now();
  merging::MergeToLineTracks(graph, tracks, all_lines_2d, imagecols, all_lines_3d, neighbors, linker);
  res->merge_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (PatchNode *n : graph.nodes) {
    res->node_img.push_back(n->image_idx);
    res->node_line.push_back((int)n->line_idx);
  }
  for (Edge *e : graph.undirected_edges) {
    res->e1.push_back((int)e->node_idx1);
    res->e2.push_back((int)e->node_idx2);
    res->sim.push_back(e->sim);
  }
  std::vector<Line3d> none;
  res->labels = merging::ComputeLineTrackLabelsGreedy(graph, none);
  res->stages[0] = tracks;
  // runners/line_fitnmerge.py:237-258
  merging::FilterSupportingLines(res->stages[1], res->stages[0], imagecols, th_angular2d, th_perp2d, 0);
  LineLinker3d rl(cr);
  std::vector<LineTrack> cur = res->stages[1];
  if (!cur.empty()) {
    size_t n = cur.size();
    while (true) {
      cur = merging::RemergeLineTracks(cur, rl, 0);
      if (cur.size() == n) break;
      n = cur.size();
    }
  }
  res->stages[2] = cur;
  merging::FilterSupportingLines(res->stages[3], res->stages[2], imagecols, th_angular2d, th_perp2d, 0);
  return res;
}

void mrg_free(void *h) { delete static_cast<Result *>(h); }
double mrg_merge_ms(void *h) { return static_cast<Result *>(h)->merge_ms; }
int mrg_max_threads(void) { return omp_get_max_threads(); }

void mrg_graph_size(void *h, int64_t *n_nodes, int64_t *n_edges) {
  Result *r = static_cast<Result *>(h);
  *n_nodes = (int64_t)r->node_img.size();
  *n_edges = (int64_t)r->e1.size();
}
void mrg_graph_get(void *h, int32_t *node_img, int32_t *node_line, int32_t *labels, int32_t *e1, int32_t *e2,
                   double *sim) {
  Result *r = static_cast<Result *>(h);
  for (size_t i = 0; i < r->node_img.size(); ++i) {
    node_img[i] = r->node_img[i]; node_line[i] = r->node_line[i]; labels[i] = r->labels[i];
  }
  for (size_t k = 0; k < r->e1.size(); ++k) { e1[k] = r->e1[k]; e2[k] = r->e2[k]; sim[k] = r->sim[k]; }
}

void mrg_stage_size(void *h, int s, int64_t *n_tracks, int64_t *n_members) {
  Result *r = static_cast<Result *>(h);
  *n_tracks = (int64_t)r->stages[s].size();
  int64_t m = 0;
  for (auto &t : r->stages[s]) m += (int64_t)t.count_lines();
  *n_members = m;
}
// line7 = start3 end3 uncertainty; line3d10 = start3 end3 depths2 uncertainty score
void mrg_stage_get(void *h, int s, double *line7, int64_t *off, int32_t *img, int32_t *lid, int32_t *nid,
                   double *score, double *line2d4, double *line3d10) {
  Result *r = static_cast<Result *>(h);
  int64_t e = 0, ti = 0;
  off[0] = 0;
  for (auto &tr : r->stages[s]) {
    double *o = line7 + 7 * ti;
    for (int k = 0; k < 3; ++k) { o[k] = tr.line.start[k]; o[3 + k] = tr.line.end[k]; }
    o[6] = tr.line.uncertainty;
    for (size_t k = 0; k < tr.count_lines(); ++k, ++e) {
      img[e] = tr.image_id_list[k]; lid[e] = tr.line_id_list[k]; nid[e] = tr.node_id_list[k];
      score[e] = tr.score_list[k];
      line2d4[4 * e] = tr.line2d_list[k].start[0]; line2d4[4 * e + 1] = tr.line2d_list[k].start[1];
      line2d4[4 * e + 2] = tr.line2d_list[k].end[0]; line2d4[4 * e + 3] = tr.line2d_list[k].end[1];
      const Line3d &l = tr.line3d_list[k];
      double *q = line3d10 + 10 * e;
      for (int c = 0; c < 3; ++c) { q[c] = l.start[c]; q[3 + c] = l.end[c]; }
      q[6] = l.depths[0]; q[7] = l.depths[1]; q[8] = l.uncertainty; q[9] = l.score;
    }
    off[++ti] = e;
  }
}

}  // extern "C"
