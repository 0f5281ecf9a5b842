// include/myslam_shim/keyframe_db_hip.inl -- the key-frame database of Map on the device (vo_kfdb):
//   Map::insertKeyFrame                    (reference src/map.cpp:9-22; the inverted-index half is :19-21)
//   Map::detectRelocalizationCandidates    (:101-208)
//   Map::detectLoopCandidates              (:210-333)
//   vo_shim::loopCandidates                detectLoop's minScore loop (src/loopClosing.cpp:68-85) and detectLoopCandidates in
//                                          one query (min_score == NULL)
// One vo_kfdb per Map, created on the first insertion and released by vo_shim::releaseKeyFrameDb(this) in Map's
// destructor.  #include at the end of map.cpp INSTEAD of the three definitions above; invertIdxs_ is no
// longer filled.  relocateScore_ / loopScore_ of the KeyFrame objects are maintained from the query's score_out, so that
// a later query sees what the reference would have left there (stale_score); relocateFrameId_ / relocateWordCnt_ /
// loopKFId_ / loopWordCnt_ are scratch of the reference's walk and are not touched.  Frame id 0 / key-frame id 0 are
// queried like any other (the reference finds nothing for them: the members' initial value collides with the id).
#include <cstdio>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "vo_hip.h"

#ifndef VO_SHIM_KFDB_MAX_KEYFRAMES
#define VO_SHIM_KFDB_MAX_KEYFRAMES 8192
#endif
#ifndef VO_SHIM_KFDB_MAX_WORDS
#define VO_SHIM_KFDB_MAX_WORDS 2048  // words of one BoW vector (a frame has at most as many as features)
#endif
#ifndef VO_SHIM_KFDB_MAX_CANDIDATES
#define VO_SHIM_KFDB_MAX_CANDIDATES 256
#endif

namespace myslam {
namespace vo_shim {

struct KeyFrameDb {
  vo_kfdb *db = nullptr;
  std::vector<KeyFrame *> kfs;                 // insertion number -> key-frame
  std::map<KeyFrame *, int> index;             // and back
  std::vector<std::vector<int32_t>> neighbors; // what the device holds per key-frame (refreshNeighbors)
};

inline std::mutex &kfdb_mutex() {
  static std::mutex m;
  return m;
}
// One database per Map.  The table is never destroyed (static destruction may run after the HIP runtime is gone); a Map
// that dies calls releaseKeyFrameDb(this) from its destructor, so that a later Map at the same address starts empty.
inline std::map<Map *, KeyFrameDb> &kfdb_table() {
  static std::map<Map *, KeyFrameDb> *dbs = new std::map<Map *, KeyFrameDb>;
  return *dbs;
}
inline KeyFrameDb &kfdb_of(Map *map) { return kfdb_table()[map]; }  // (callers hold kfdb_mutex())
inline void releaseKeyFrameDb(Map *map) {
  std::lock_guard<std::mutex> lock(kfdb_mutex());
  auto it = kfdb_table().find(map);
  if (it == kfdb_table().end()) return;
  vo_kfdb_destroy(it->second.db);
  kfdb_table().erase(it);
}
// the reference has no error channel: what the shim cannot do is said on stderr, once per kind
inline void complain(const char *what) {
  static std::set<std::string> said;
  if (said.insert(what).second) fprintf(stderr, "myslam_shim key-frame database: %s (%s)\n", what, vo_last_error());
}

inline void flatten(const DBoW3::BowVector &v, std::vector<int32_t> &w, std::vector<double> &x) {
  w.clear(), x.clear();
  for (const auto &e : v) w.push_back((int32_t)e.first), x.push_back(e.second);  // std::map: ascending word ids
}

// KeyFrame::getBestCovisibleKFs(10) changes as the map grows: before a query the lists are read again on the host and the
// span of key-frames whose list differs from what the device holds goes up in ONE call (vo_kfdb_set_neighbors_batch: two
// copies, no launch per key-frame).  The reference asks only the scored key-frames, which are not known before the query:
// the host loop over all key-frames stays, the device traffic does not grow with it.
inline void refreshNeighbors(KeyFrameDb &D) {
  const size_t N = D.kfs.size();
  D.neighbors.resize(N);
  size_t lo = N, hi = 0;
  std::vector<int32_t> ids;
  for (size_t k = 0; k < N; k++) {
    ids.clear();
    for (KeyFrame *n : D.kfs[k]->getBestCovisibleKFs(10)) {
      auto it = D.index.find(n);
      if (it != D.index.end() && ids.size() < 10) ids.push_back(it->second);
    }
    if (ids == D.neighbors[k]) continue;
    D.neighbors[k] = ids;
    lo = k < lo ? k : lo, hi = k + 1;
  }
  if (lo >= hi) return;
  std::vector<int32_t> n(hi - lo), rows((hi - lo) * 10, -1);
  for (size_t k = lo; k < hi; k++) {
    n[k - lo] = (int32_t)D.neighbors[k].size();
    for (size_t i = 0; i < D.neighbors[k].size(); i++) rows[(k - lo) * 10 + i] = D.neighbors[k][i];
  }
  if (vo_kfdb_set_neighbors_batch(D.db, (int)lo, (int)(hi - lo), n.data(), rows.data()) != VO_OK) {
    complain("vo_kfdb_set_neighbors_batch failed");
    for (size_t k = lo; k < hi; k++) D.neighbors[k].assign(1, -2);  // unknown on the device: sent again next time
  }
}

inline std::vector<KeyFrame *> toKeyFrames(const KeyFrameDb &D, int n, const std::vector<int32_t> &cand) {
  std::vector<KeyFrame *> out;
  for (int i = 0; i < n; i++) out.push_back(D.kfs[cand[i]]);
  return out;
}

// VO_ERR_CAPACITY from a query with more than VO_SHIM_KFDB_MAX_CANDIDATES candidates still leaves the first
// VO_SHIM_KFDB_MAX_CANDIDATES of them and score_out in place: they are used (the members stay in step with the reference) and
// the cut is reported.  Any other failure: "no candidates", reported.
inline bool queryUsable(int rc, int32_t &n) {
  if (rc == VO_OK) return true;
  if (rc == VO_ERR_CAPACITY && n > VO_SHIM_KFDB_MAX_CANDIDATES) {
    complain("more candidates than VO_SHIM_KFDB_MAX_CANDIDATES, list cut");
    n = VO_SHIM_KFDB_MAX_CANDIDATES;
    return true;
  }
  complain("query failed, no candidates returned");
  return false;
}

// detectLoop :68-85: minScore over the non-bad orderedConnectKFs_, then detectLoopCandidates, as one device query
inline std::vector<KeyFrame *> loopCandidates(Map *map, KeyFrame *keyframe, const float *minScore) {
  std::lock_guard<std::mutex> lock(kfdb_mutex());
  KeyFrameDb &D = kfdb_of(map);
  if (!D.db || D.kfs.empty()) return std::vector<KeyFrame *>();
  refreshNeighbors(D);
  std::vector<int32_t> qw, excl, conn, cand(VO_SHIM_KFDB_MAX_CANDIDATES);
  std::vector<double> qv;
  flatten(keyframe->bowVec_, qw, qv);
  std::set<KeyFrame *> connect = keyframe->getConnectKFs();
  connect.insert(keyframe);
  for (KeyFrame *kf : connect) {
    auto it = D.index.find(kf);
    if (it != D.index.end()) excl.push_back(it->second);
  }
  if (!minScore)
    for (KeyFrame *kf : keyframe->orderedConnectKFs_) {
      auto it = D.index.find(kf);
      if (!kf->isBad() && it != D.index.end()) conn.push_back(it->second);
    }
  const int32_t q_start[2] = {0, (int32_t)qw.size()}, e_start[2] = {0, (int32_t)excl.size()}, c_start[2] = {0, (int32_t)conn.size()};
  std::vector<float> scores(D.kfs.size());
  int32_t n = 0;
  const int rc = vo_kfdb_query_loop(D.db, 1, q_start, qw.data(), qv.data(), e_start, excl.data(), minScore, c_start, conn.data(),
                                    VO_SHIM_KFDB_MAX_CANDIDATES, &n, cand.data(), scores.data());
  if (!queryUsable(rc, n)) return std::vector<KeyFrame *>();
  for (size_t k = 0; k < D.kfs.size(); k++)
    if (scores[k] >= 0.0f) D.kfs[k]->loopScore_ = scores[k];  // -1: not scored by this query
  return toKeyFrames(D, n, cand);
}

}  // namespace vo_shim

void Map::insertKeyFrame(KeyFrame *keyframe) {
  {
    unique_lock<mutex> lock(mutexMap_);
    keyframes_.insert(keyframe);
  }
  if (keyframe->id_ > maxKFId_) maxKFId_ = keyframe->id_;
  std::lock_guard<std::mutex> lock(vo_shim::kfdb_mutex());
  vo_shim::KeyFrameDb &D = vo_shim::kfdb_of(this);
  if (!D.db) {
    if (!voc_ || voc_->size() == 0) return vo_shim::complain("Map::voc_ is not set, key-frame not indexed");
    if (vo_kfdb_create(&D.db, (int)voc_->size(), VO_SHIM_KFDB_MAX_KEYFRAMES, VO_SHIM_KFDB_MAX_WORDS, 1) != VO_OK)
      return vo_shim::complain("vo_kfdb_create failed, key-frame not indexed");
  }
  std::vector<int32_t> w;
  std::vector<double> x;
  vo_shim::flatten(keyframe->bowVec_, w, x);
  int32_t idx = -1;
  if (vo_kfdb_insert(D.db, (int)w.size(), w.data(), x.data(), &idx) != VO_OK)
    return vo_shim::complain("vo_kfdb_insert failed (VO_SHIM_KFDB_MAX_KEYFRAMES / VO_SHIM_KFDB_MAX_WORDS?), key-frame not indexed");
  D.kfs.push_back(keyframe);
  D.index[keyframe] = idx;
}

vector<KeyFrame *> Map::detectRelocalizationCandidates(Frame *frame) {
  std::lock_guard<std::mutex> lock(vo_shim::kfdb_mutex());
  vo_shim::KeyFrameDb &D = vo_shim::kfdb_of(this);
  if (!D.db || D.kfs.empty()) return vector<KeyFrame *>();
  vo_shim::refreshNeighbors(D);
  std::vector<int32_t> qw, cand(VO_SHIM_KFDB_MAX_CANDIDATES);
  std::vector<double> qv;
  vo_shim::flatten(frame->bowVec_, qw, qv);
  std::vector<float> stale(D.kfs.size()), scores(D.kfs.size());
  for (size_t k = 0; k < D.kfs.size(); k++) stale[k] = D.kfs[k]->relocateScore_;
  const int32_t q_start[2] = {0, (int32_t)qw.size()};
  int32_t n = 0;
  const int rc = vo_kfdb_query_reloc(D.db, 1, q_start, qw.data(), qv.data(), stale.data(), VO_SHIM_KFDB_MAX_CANDIDATES, &n,
                                     cand.data(), scores.data());
  if (!vo_shim::queryUsable(rc, n)) return vector<KeyFrame *>();
  for (size_t k = 0; k < D.kfs.size(); k++) D.kfs[k]->relocateScore_ = scores[k];
  return vo_shim::toKeyFrames(D, n, cand);
}

vector<KeyFrame *> Map::detectLoopCandidates(KeyFrame *keyframe, float minScore) {
  return vo_shim::loopCandidates(this, keyframe, &minScore);
}

}  // namespace myslam
