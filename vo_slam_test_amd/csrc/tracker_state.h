// tracker_state.h -- the tracker's handle as its own files see it (not part of the C-ABI): tracker.hip (the routes, the
// setters, the getters), handover.hip (frame_last_ = frame_curr_ on the device), motion_store.hip (the
// motion route's local map, point counters and pose refresh from the key-frame store, section 4v) and handover_store.hip (the
// hand-over and the counters behind the relocalisation and reference-key-frame routes from the store, section 4w).
#pragma once
#include "kfstore.h"

#include <vector>

namespace vo {

// What a call runs: the front (extraction + Frame::Frame), one of the two first stages -- trackWithMotion's projection
// search (with its 2 x radius retry) or trackRefKeyFrame's vocabulary-node search --, and the local-map stage.
enum : unsigned { kRunFront = 1u, kRunMotion = 2u, kRunRefKeyFrame = 4u, kRunLocal = 8u, kRunReloc = 16u, kRunRefStore = 32u };

// handover.hip's device block (motion_store.hip reads the last ids, the poses and the sort keys of it) and what tracker.hip
// needs of it
struct Handover {
  Arena mem;
  int P = 0;  // the power of two >= max_features: the keys of a frame
  int *slot_ids = nullptr, *last_ids = nullptr, *motion_state = nullptr, *temp_count = nullptr;
  uint8_t *slot_desc = nullptr, *slot_flags = nullptr, *last_valid = nullptr;
  double *frame_pose = nullptr, *velocity = nullptr, *last_pose = nullptr;  // last_pose: [B][12], then last_valid [B]
  unsigned long long *keys = nullptr;                                        // [B][P] where P > kHoLdsKeys, else unused
};
constexpr int kHoLdsKeys = 4096;
void handover_destroy(Handover *h);
int handover_ensure(vo_tracker *t);  // the block, allocated and cleared by the first call that needs it
// device array behind one of the selectors from VO_TRACKER_SLOT_IDS on (nullptr: not one of them, or not there yet)
const void *handover_selector(const vo_tracker *t, int what, size_t *bytes);

// motion_store.hip's device block and what tracker.hip needs of it.  vo_tracker_build_local_map on the
// motion route: motion_store_ensure before anything is enqueued; motion_store_slot_ids enqueues the gather and points the
// builder's arguments at the ids and at a vote mask of their own (a temporary point holds a point and no id: it must neither
// vote nor be nulled); motion_store_link, behind the builder, takes the nulling over into the tracker's slots and writes `link`.
struct MotionStore;
void motion_store_destroy(MotionStore *m);
int motion_store_ensure(vo_tracker *t);
int motion_store_slot_ids(vo_tracker *t, LocalMapArgs *A, hipStream_t st);
int motion_store_link(vo_tracker *t, hipStream_t st);
// device array behind one of the selectors from VO_TRACKER_FIRST_SLOT_IDS on (nullptr: not one of them, or not there yet)
const void *motion_store_selector(const vo_tracker *t, int what, size_t *bytes);
// the three counter arrays [B][row] of the block (handover_store.hip fills the rows vo_tracker_point_stats_arrays hands out)
void motion_store_stat_rows(const vo_tracker *t, int **ids, int **visible, int **found, int *row);

}  // namespace vo

struct RefKfHost {
  int n = 0;
  std::vector<uint8_t> valid, desc;
  std::vector<float> angle;
  std::vector<int32_t> node_id, start;
  std::vector<uint32_t> feat;
  vo_bow_view view{};
};

struct vo_tracker {
  vo_tracker_config cfg{};
  vo_orb *orb = nullptr;
  vo_frames *frames = nullptr;
  hipStream_t st = nullptr, est = nullptr;
  bool own_st = false, own_est = false;
  hipEvent_t ev_extract = nullptr, ev_build = nullptr;
  // host-buffer calls: the depth image is first read BEHIND the extraction (vo_frames_build_dev), so its upload goes on a copy
  // stream of its own, issued after the extraction has been enqueued: the key-points are being extracted while the host (pageable
  // memory: the runtime stages it synchronously) and the copy engine move the depth -- two thirds of the bytes of a frame
  hipStream_t cst = nullptr;
  hipEvent_t ev_depth = nullptr;
  const void *pend_depth = nullptr;
  size_t pend_depth_bytes = 0;
  bool have_build = false;
  int B = 0, kcap = 0, cap = 0, n_levels = 0, n_last = 0, n_local = 0, nq_last = 0, nq_local = 0;
  float sf[16] = {0};
  // device state
  // device state: every array below is sized from (B, kcap, cap, n_last, n_local) at creation and lives in one block (`mem`,
  // laid out by layout()) except the extraction's output; the images and depth of the host-buffer calls grow with those calls
  vo::Arena mem;
  struct Arrays {
    vo_keypoint *kps;  // extraction: [B][kcap] key-points, descriptors, [B] counts
    uint8_t *desc;
    int *cnt;
    uint8_t *q0_flags, *q0_desc, *pf0, *last_matched;  // the last frame's map points as queries [B][n_last]
    float *q0_u, *q0_v, *q0_aux, *q0_angle;
    int *q0_level;
    double *p0;
    uint8_t *q1_flags, *q1_desc, *pf1;  // the local map's [B][n_local]
    float *q1_u, *q1_v, *q1_aux, *q1_viewcos, *mind1, *maxd1;
    int *q1_level, *link1, *ids1;  // ids1: map-point ids of the local points (vo_tracker_set_local_map_ids)
    double *p1, *nrm1;
    double *Tcw, *pose0, *pose, *pose_first;  // Tcw: [B][12], then the intrinsics as doubles
    uint8_t *resblk;                          // k_track_pack's block (72 bytes per frame + 2 flags)
    int *retry_nq;                            // [B] query counts of the retry pass
    int *store_err;                           // the store routes' sticky word (vo_common.h: kStoreErr*)
    int *ref_kf;                              // [B] the key-frame numbers of the last trackRefKeyFrame from the store
    int *assigned, *assigned_first, *nm, *nm_first, *ninl, *ninl_first, *nobs_first, *ntracked, *status;
    double *fpoint, *pts, *obs, *isg;  // per-feature frame state [B][cap] and the pose problem gathered from it
    uint8_t *fhas, *fobs, *foutl, *outlier;
    int *ranges, *index;
  } d{};
  void layout(vo::Arena &a);
  vo::OwnedDevBuf images, depth;
  vo::OwnedDevBuf kps, desc;  // d.kps, d.desc: allocations of their own -- inside the block the headline measured 0.4 % slower
  vo::OwnedPinnedBuf stage;
  bool have_result = false;  // a call has written the result block
  bool have_link = false;
  bool have_local = false, have_ids = false;  // vo_tracker_set_local_map / _ids have been called (the ids belong to that local map)
  bool last_reloc = false;                    // the last front ran a relocalisation route: track_local_map takes the hand-over
  // vo_tracker_build_local_map: which slot ids the last front left (0: none; 1: a relocalisation from the store; 2:
  // trackRefKeyFrame from the store, first stage only); its buffers, laid out by the first call for the store's max_keyframes
  int ids_route = 0;
  vo::Arena lm_mem;
  int lm_max_kf = 0;
  struct { int *votes, *lkf, *n_kf, *best, *n_pts; } lm{};
  // a search's matches that the next solve_pose writes into the frame's slots (k_track_scatter_gather)
  struct { const int32_t *assigned = nullptr; const double *qpoints = nullptr; const uint8_t *qflags = nullptr; int stride = 0; } pend;
  int first_min_matches = 20;
  // trackRefKeyFrame's reference key-frame per frame of the batch (host copies: the common-node walk is host work)
  const vo_vocab *ref_vocab = nullptr;
  std::vector<RefKfHost> ref_kf;
  // the relocalisation route (reloc.hip); NULL: not configured (vo_tracker_config.max_reloc_candidates == 0)
  vo::Reloc *reloc = nullptr;
  const vo::RelocStoreArgs *store_args = nullptr;  // set for the duration of a vo_tracker_relocalize_store / _db call
  // the store routes' BoW walk buffers (relocalisation and trackRefKeyFrame share them), sized by the first such call
  vo::BowWalkBufs walk;
  // trackRefKeyFrame from the store: the arguments of the call being enqueued; whether the last front ran that route
  struct RefStoreArgs { const vo_kfstore *store; const vo_vocab *vocab; const int32_t *ref_kf; const double *Tcw12; };
  const RefStoreArgs *ref_store_args = nullptr;
  bool ref_store = false;
  const char *store_call = "";                      // the entry point of the last store route (error texts)
  hipEvent_t rtev[8] = {nullptr};                   // vo_tracker_get_reloc_timing: created by the first timed store route
  bool rtimed = false;
  // the hand-over (handover.hip): the stages the last track call ran to its end (kRun* bits, 0: none, or it failed); whether the
  // last-frame list carries ids (vo_tracker_set_last_frame_ids, vo_tracker_end_frame); whether that list is the frame
  // vo_tracker_end_frame handed over, still in the frame store's slots (no track call and no setter since); the block
  unsigned last_run = 0;
  bool have_last_ids = false, handed_over = false;
  vo::Handover *ho = nullptr;
  // the motion route from the store (motion_store.hip): the block; whether vo_tracker_build_local_map has built this frame's map
  // from the last ids (VO_TRACKER_FIRST_SLOT_IDS is the frame's; vo_tracker_results reads the store routes' sticky word);
  // whether the local-map stage ran as a call of its own (vo_tracker_track_local_map); whether vo_tracker_begin_frame has run
  // since vo_tracker_end_frame (the window of vo_tracker_refresh_last_pose)
  vo::MotionStore *ms = nullptr;
  bool lm_motion = false, local_split = false, begun = false;
  // the hand-over behind the store's other two routes (handover_store.hip, section 4w): the ids_route whose frame
  // vo_tracker_build_local_map built the present local map for (0: none -- set by the host, or the motion route's); whether
  // vo_tracker_track_local_map has run since (on either branch)
  int lm_route = 0;
  bool local_ran = false;
  // timing
  bool timing = false;
  // 2 events per stage and timed call, in a list that grows with the calls; they are read (after one synchronisation) only
  // by vo_tracker_get_timing, never inside a track call: a timed call enqueues exactly like an untimed one
  std::vector<hipEvent_t> tev;
  int tissued = 0;   // timed calls whose events are recorded and not yet read
  int tslot = -1;    // event set of the call being enqueued (-1: not timed)
  double tms[VO_TRACKER_STAGES] = {0};
  int tcalls = 0;
};
