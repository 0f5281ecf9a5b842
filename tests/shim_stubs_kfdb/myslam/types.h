// stub declarations for include/myslam_shim/keyframe_db_hip.inl: overrides ../../shim_stubs/myslam/types.h (found first on
// the include path) with the members of KeyFrame, Frame and Map that the key-frame database shim touches
#pragma once
#include <DBoW3/DBoW3.h>
#include "myslam/common_include.h"
namespace myslam {
class KeyFrame {
 public:
  unsigned long id_; DBoW3::BowVector bowVec_; vector<KeyFrame *> orderedConnectKFs_;
  unsigned long relocateFrameId_; int relocateWordCnt_; float relocateScore_;
  unsigned long loopKFId_; int loopWordCnt_; float loopScore_;
  vector<KeyFrame *> getBestCovisibleKFs(const int &N); set<KeyFrame *> getConnectKFs(); bool isBad();
};
class Frame {
 public:
  unsigned long id_; DBoW3::BowVector bowVec_;
};
class Map {
 public:
  set<KeyFrame *> keyframes_; DBoW3::Vocabulary *voc_; unsigned long maxKFId_; mutex mutexMap_;
  void insertKeyFrame(KeyFrame *keyframe);
  vector<KeyFrame *> detectRelocalizationCandidates(Frame *frame);
  vector<KeyFrame *> detectLoopCandidates(KeyFrame *keyframe, float minScore);
};
}  // namespace myslam
