// kfstore.h -- the key-frame feature store as its own files see it (DESIGN.md sections 4f-4t; not part of the C-ABI): the
// kernel-argument views of the store and of its opt-in layers, the functions a layer's file shares with another file, the
// handle itself, and the guards every entry point starts with.  Included by kfstore.hip, by the layer files and by the
// store's readers (match.hip, reloc.hip, tracker.hip, local_map.hip).
#pragma once
#include "vo_common.h"

namespace vo {

// ---- the key-frame feature store (kfstore.hip).  One fixed-size record per key-frame, every
// section at a fixed byte offset: [n, bad, n_nodes, 0 | angle | min_distance | max_distance | ids | node | start | feat |
// points | desc | point_desc | flags], NK entries per section (start: NK + 1).  A record is one contiguous copy for the
// host insert; kernels address a section as base + k * rec + offset.
struct KfStoreView {
  int size, max_kf, NK;
  size_t rec;
  const uint8_t *base;
  size_t o_angle, o_mind, o_maxd, o_ids, o_node, o_start, o_feat, o_points, o_desc, o_pdesc, o_flags;
};
__host__ __device__ __forceinline__ const int *kf_head(const KfStoreView &V, int k) {
  return reinterpret_cast<const int *>(V.base + (size_t)k * V.rec);
}
template <class T>
__host__ __device__ __forceinline__ const T *kf_sec(const KfStoreView &V, int k, size_t off) {
  return reinterpret_cast<const T *>(V.base + (size_t)k * V.rec + off);
}
KfStoreView kfstore_view(const vo_kfstore *s);
// `st` waits for what the store's stream holds now / the store's stream waits for what `st` holds now (events, no host wait)
int kfstore_order_before(const vo_kfstore *s, hipStream_t st);
int kfstore_order_after(const vo_kfstore *s, hipStream_t st);

// What vo_tracker_build_local_map reads beyond the records (kfstore.hip).  graph: kKfGraphInts ints
// per key-frame [n_neighbors, n_children, parent, 0 | neighbors 10, 2 spare | children 64]; normals [max_kf][NK][3]; the
// observation index: keys [n_keys] ascending, key = map-point id << 32 | entry, entry = key-frame * NK + feature, for the
// features with flags bit 0 set (~0ull: no entry; n_keys a power of two >= 2048); run[entry] = position of the first key
// of the entry's id.  kfstore_obs_view rebuilds the index on the store's stream when an insert or update_points has
// happened since the last use (launches only), and returns the views.
constexpr int kKfGraphNb = VO_KFSTORE_MAX_NEIGHBORS, kKfGraphCh = VO_KFSTORE_MAX_CHILDREN, kKfGraphInts = 16 + kKfGraphCh;
struct KfObsView {
  const int *graph;
  const double *normals;
  const unsigned long long *keys;
  const int *run;
  int n_keys;
};
int kfstore_obs_view(vo_kfstore *s, KfObsView *out);

// The covisibility graph and spanning tree of a store, maintained on the device (connections.hip):
// KeyFrame::updateConnections (keyframe.cpp:69-152) for a device list of key-frame numbers, in list order.  The state is
// allocated once by vo_kfstore_enable_connections (over the store's graph rows, which the calls rewrite);
// connections_reserve sizes the scratch of a list of n entries (grow-only) and returns the device list of the host form;
// connections_update enqueues three launches on st and nothing else.
struct KfConnections;
void connections_destroy(KfConnections *c);
int connections_reserve(KfConnections *c, int n, int **dev_list);
int connections_update(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n, const int *dev_list, hipStream_t st);
// for the culling kernels (cull.hip): the state's arrays; the `erased` column every later update and ordering pass
// honours (NULL until vo_kfstore_enable_culling); k_conn_order over the touched key-frames on its own (one launch)
struct KfConnView {
  int max_kf;
  int *W, *ordered, *n_ordered, *mode, *parent, *touched, *status;
};
KfConnView connections_view(const KfConnections *c);
// for the loop correction (loop_correct.hip), whose list and length only the device knows.  n_max: the
// entries the launches are sized for (reserved beforehand); dev_n: how many of them count -- the rest is skipped without a
// sticky bit.  connections_update_counted is connections_update for such a list.  connections_update_rows also writes, per
// list position t, out[t * max_kf + j] = 1 for the key-frames j that update(list[t]) connects list[t] to -- the weight row as
// the step leaves it, less the members of list[t]'s ordered list as the step FOUND it, less the key-frames with listed[j] != 0
// (loopClosing.cpp:461-479); the connection state afterwards is connections_update's.
int connections_update_counted(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n_max, const int *dev_list, const int *dev_n,
                               hipStream_t st);
int connections_update_rows(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n_max, const int *dev_list, const int *dev_n,
                            const int *listed, uint8_t *out, hipStream_t st);
void connections_set_erased(KfConnections *c, const int *erased);
int connections_order(KfConnections *c, int size, hipStream_t st);

// Key-frame culling on the device (cull.hip): LocalMapping::cullingKeyFrames with
// KeyFrame::eraseKeyFrame, eraseConnection and MapPoint::eraseObservedKF.  cols: [max_kf][3][NK] -- octave (int32), depth,
// u_right (float) of a key-frame side by side, so that the host form of set_keypoints is one copy; erased, locked, pending
// [max_kf]; rec [max_kf] (key-frame, mp_cnt, re_obs, decision) of the last cull call and n_rec its candidate count.
struct KfCullView {
  int NK;
  int *cols;
  int *erased, *locked, *pending, *n_rec;
  int4 *rec;
};
__host__ __device__ __forceinline__ int *cull_octave(const KfCullView &X, int k) { return X.cols + (size_t)k * 3 * X.NK; }
__host__ __device__ __forceinline__ float *cull_depth(const KfCullView &X, int k) {
  return reinterpret_cast<float *>(X.cols + ((size_t)k * 3 + 1) * X.NK);
}
__host__ __device__ __forceinline__ float *cull_uright(const KfCullView &X, int k) {
  return reinterpret_cast<float *>(X.cols + ((size_t)k * 3 + 2) * X.NK);
}

// New map points on the device (new_points.hip, match.hip): LocalMapping::createNewMapPoints.  What
// vo_kfstore_enable_mapping allocates, one block: pose [max_kf][13] doubles (R row-major, t, and in the thirteenth slot the
// pose-set word, so that the host form of set_pose is one copy); xy [max_kf][2][NK] (unKeypoints_[i].pt: a key-frame's x
// column, then its y column -- split so that k_node_replay reads them as it reads a frame view's, side by side so that the
// host form of set_keypoint_xy is one copy); the id counter;
// rec, the result record: [n_neighbors, created in all, 0, 0 | (key-frame, status, n_matches, n_created) x 10]; created
// [10][NK] rows (key-frame, idx1, idx2, id); and the scratch of ONE neighbour step: query list, claims, the argument block
// of k_node_replay (match.hip's NodeArgs: tri_args_bytes), the neighbour's claimable bytes, match12, the match count and
// the step's geometry.
constexpr int kNpRecInts = 4 + 4 * VO_KFSTORE_MAX_NEIGHBORS;
struct NpStep {
  double T1[12], T2[12], Ow1[3], Ow2[3], F[9];
  float ex, ey, bl;
  int kf, status;
};
struct KfMapView {
  int NK, n_levels;
  float cam[6], sf[16];  // fx, fy, cx, cy, bf, b; scaleFactors_ (entries beyond n_levels repeat the last)
  double *pose;
  float *xy;
  int *counter, *rec;
  int4 *created, *queries, *claims;
  uint8_t *args, *bok;
  int *match, *nm;
  NpStep *step;
};
constexpr int kNpPoseDoubles = 13;
__host__ __device__ __forceinline__ double *np_pose(const KfMapView &M, int k) { return M.pose + (size_t)k * kNpPoseDoubles; }
__host__ __device__ __forceinline__ int *np_pose_set(const KfMapView &M, int k) { return reinterpret_cast<int *>(np_pose(M, k) + 12); }
__host__ __device__ __forceinline__ float *np_x(const KfMapView &M, int k) { return M.xy + (size_t)k * 2 * M.NK; }
__host__ __device__ __forceinline__ float *np_y(const KfMapView &M, int k) { return M.xy + ((size_t)k * 2 + 1) * M.NK; }
// one neighbour step = three launches.  tri_walk_replay (match.hip): k_tri_walk -- the step's neighbour from `current`'s
// graph row, its status and geometry (new_points_geom.h), the record's entry (the whole record on step 0), the store-to-
// store common-node walk and the argument block -- then k_node_replay in triangulation mode; `status`: the store's sticky
// word.  k_np_create (new_points.hip) follows.
size_t tri_args_bytes();
int tri_walk_replay(const KfStoreView &S, const KfCullView &X, const KfMapView &M, const int *graph, int *status, int current, int step,
                    hipStream_t st);

// Local BA from the store (local_ba_store.hip): the window of Optimizer::solveLocalBAPoseAndPoint
// (optimizer_ceres.cpp:449-592) assembled from the observation index, its write-back (:757-804) and
// MapPoint::updateNormalAndDepth (mappoint.cpp:66-116).  What vo_kfstore_enable_local_ba allocates, one block: ref_kf
// [max_kf][NK] (MapPoint::keyFrame_ref_ per feature, -1: unknown); mark / fixm / lcam [max_kf] (camera index + 1 of a
// key-frame, -1: marked local but bad; "holds a local point without being local"; the local cameras in list order); blk, the
// first-occurrence count of every workgroup of the point grid; pt_ne [max_points + 1], edges per point, then their exclusive
// offsets; dead [max_points]; ids_in [max_points], refresh_points' list; the WINDOW, contiguous so that one copy fetches it:
// rec (kBaRecInts ints: n_cams, n_local, n_fixed, n_points, n_edges, n_dropped, status, current, n_erased, n_feature0, n_dead),
// cam_kf, cam_fixed, poses6, pt_id, points, e_cam, e_pt, e_feat, e_obs, e_isg; and `in`, the apply's inputs as the one staging
// copy brings them: Tcw12 per camera | points | erase bytes, packed by the window's counts.
constexpr int kBaRecInts = 16;
enum { kBaNCams = 0, kBaNLocal, kBaNFixed, kBaNPoints, kBaNEdges, kBaNDropped, kBaStatus, kBaCurrent, kBaNErased, kBaNFeature0, kBaNDead };
struct KfBaView {
  int max_cams, max_points, max_edges, NK;
  int *ref_kf, *mark, *fixm, *lcam, *blk, *pt_ne, *ids_in;
  uint8_t *dead;
  uint8_t *win;
  size_t win_bytes;
  int *rec, *cam_kf;
  uint8_t *cam_fixed;
  double *poses6;
  int *pt_id;
  double *points;
  int *e_cam, *e_pt, *e_feat;
  double *e_obs, *e_isg;
  uint8_t *in;
  size_t in_bytes;
};
// the refresh for the n entries of a device list; a negative entry is skipped (point_upkeep.hip's tracked points)
int ba_refresh_list_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                            double *normals, int *status, int n, const int *dev_ids, hipStream_t st);

// Map-point upkeep on the device (point_upkeep.hip): LocalMapping::processNewKeyFrame,
// cullingMapPoints, MapPoint::computeDescriptor and eraseMapPoint from the store.  What vo_kfstore_enable_point_upkeep
// allocates, one block (R = max_recent, L = R + NK, the longest id list a call takes): head [4] (entries in the recent
// list, ids in the overflow list, the key-frame number process_new_keyframe hands to the connection update, 0); the recent
// list id / first_kf / found / visible [R] each (addedMapPoints_ with firstAddedIdxofKF_, found_cnt_, visible_cnt_); rec
// [kUpRecInts] and erased [R], the last call's record and the ids it erased; list [3][L], the id list of a call (the host
// forms' one copy lands here: ids | visible | found); over [L], the ids whose holders exceed a wavefront; cand [NK], the
// ids process_new_keyframe may append; outcome [R], a cull call's branch per entry.
constexpr int kUpRecInts = 16;
enum { kUpKind = 0, kUpCurrent, kUpNTracked, kUpNNew, kUpNAppended, kUpNDead, kUpNRatio, kUpNFewObs, kUpNMatured, kUpNKept, kUpNErased,
       kUpNRecent };
constexpr int kUpDescMaxHolders = VO_KFSTORE_DESC_MAX_HOLDERS;
struct KfUpkeepView {
  int R, NK, L;
  int *head, *id, *first_kf, *found, *visible, *rec, *erased, *list, *over, *cand, *outcome;
};
// computeDescriptor for the n entries of a device list (negative: skipped): a memset of the overflow count and two launches
int upkeep_descriptors_enqueue(const KfStoreView &S, const KfObsView &O, const KfUpkeepView &U, int *status, int n, const int *dev_ids,
                               hipStream_t st);
// addedMapPoints_.push_back for the points create_map_points has just created for `current`
int upkeep_created_enqueue(const KfMapView &M, const KfUpkeepView &U, int *status, int current, hipStream_t st);

// Map-point fusion on the device (fuse.hip): LocalMapping::searchInNeighbors, Matcher::fuseMapPoints
// and MapPoint::replaceMapPoint from the store.  What vo_kfstore_enable_fuse allocates, one block.  The OVERLAY on the
// observation index as it stood at the start of a call (n_slots = the index's capacity; a slot is addressed by the start of
// an id's run, values are stored + 1 so that a memset resets them): m_next / m_tail, per root the chain of the runs of the ids
// a replace has merged into it; a_head with node_entry / node_next [M], per id the entries a call has added to it (a match
// reserves the node of its own number).  first [n_slots]: the first occurrence of an id in a step's list.  head [4]: targets
// in the list, matches reserved by the call, `current`, the length of the closing step's list; base [64]: head[1] at the
// start of a step; targets [64]; rec [64][8]: (target, passed, matches, adds, kept_org, kept_candidate, cleared, undone) per
// step; snap [NK], `current`'s ids at the start; list [60 NK], a step's candidates; mt [M], the matches (list position, id,
// slot, feature) and key [M], their chain keys.
constexpr int kFuseSteps = 61, kFuseRecInts = 8, kFuseFinal = 60, kFuseMaxCarriers = VO_KFSTORE_FUSE_MAX_CARRIERS;
enum { kFuTarget = 0, kFuPassed, kFuMatches, kFuAdds, kFuKeptOrg, kFuKeptCand, kFuCleared, kFuUndone };
struct KfOverlay {
  int n_slots, n_nodes;
  int *m_next, *m_tail, *a_head, *node_entry, *node_next;
};
struct KfFuseView {
  int NK, M, list_cap;
  float xmin, xmax, ymin, ymax, gpw, gph;
  KfOverlay V;
  int *first, *head, *base, *targets, *rec, *snap, *list, *key;
  int4 *mt;
  size_t reset_bytes;  // from the block's start: everything a call resets
};
struct FuseArgs {
  KfStoreView S;
  KfObsView O;
  KfConnView C;
  KfCullView X;
  KfMapView M;
  KfBaView B;
  KfUpkeepView U;
  KfFuseView F;
  double *normals;
  int *status;
};

// Loop Sim3 on the device (loop_sim3.hip, match.hip, sim3.hip): LoopClosing::computeSim3 from the
// store.  What vo_kfstore_enable_loop allocates, one block (C = max_candidates, P = max_loop_points, n_slots = the observation
// index's capacity).  st [kLoopStateInts]: the record (entries 0 .. 8, include/vo_hip.h) and the walk's own words (enum below);
// cand [16]; rand [max_rand]; iters [NK + 1], ransacMaxIters by N, tabulated on the host; per [16][8]; the FRONT, per
// candidate: queries / claims [NK], k_node_replay's argument block, bok [NK] (features of the candidate that may be claimed),
// match12 [NK] (searchByBoW's result: feature of the candidate per feature of `current`), nm; the SOLVERS, per candidate:
// pc1 / pc2 [NK][3], px1 / px2 [NK][2], me1 / me2 / midx [NK] (Sim3Solver's pcams, pixels, maxError and matchedIndexs_);
// tflags [5][NK], the inlier flags of the up-to-five trips of one iterate call; a VERIFICATION: inl [NK] (inlierMappoints as
// features of the candidate, -1: null), m2on [NK] (matched2), m1 / m2 [NK] (searchBySim3's two directions), the refinement's
// inputs Pm Pc [NK][3], pxc pxm [NK][2], isc ism [NK], sidx [NK], off [2], pose [6], scale, outl [NK], ninl, sums [2]; Scm,
// Scw [13]; AFTER a match: mark [n_slots] (the first list position of an id), fnd [n_slots] bytes (the id is in
// matchMapPoints_), loop_ids [P] with their list positions qg [P] and the projection's qu qv qlv qok [P], and match_ids [NK].
constexpr int kLoopStateInts = 32, kLoopPerInts = 8, kLoopTrips = 5;
enum { kLsState = 0, kLsMatchPos, kLsMatchKf, kLsRounds, kLsVerifs, kLsRandUsed, kLsRefine, kLsMatchCnt, kLsNLoop,
       kLsCurrent = 16, kLsNCand, kLsFixScale, kLsNRand, kLsRandMax, kLsCursor, kLsLive, kLsPhase, kLsPending, kLsNCur };
enum { kLoopWalk = 0, kLoopVerify, kLoopAfter, kLoopDone, kLoopHalt };  // st[kLsPhase]
enum { kLpKf = 0, kLpReason, kLpBow, kLpN, kLpMaxIters, kLpIters, kLpBest, kLpVerifs };
struct KfLoopView {
  int NK, C, P, max_rand, n_slots;
  int *st, *cand, *rand, *iters, *per;
  int4 *queries, *claims;
  uint8_t *args, *bok;
  int *match12, *nm;
  double *pc1, *pc2, *px1, *px2;
  int *me1, *me2, *midx;
  uint8_t *tflags;
  int *inl, *m1, *m2, *sidx, *off, *ninl;
  uint8_t *m2on, *outl;
  double *Pm, *Pc, *pxc, *pxm, *isc, *ism, *pose, *scale, *Scm, *Scw, *cam4;
  vo_lm_summary *sums;
  unsigned *mark;
  uint8_t *fnd, *qok;
  int *loop_ids, *qlv, *qg, *match_ids;
  float *qu, *qv;
};
struct LoopArgs {
  KfStoreView S;
  KfObsView O;
  KfConnView C;
  KfCullView X;
  KfMapView M;
  KfFuseView F;  // the image bounds and the grid pitch
  KfLoopView L;
  int *status;
};
// the front's searchByBoW(current, cand[c], mode 1, checkRot) for c < n_cand in ONE k_node_replay launch (match.hip)
int loop_bow_replay(const LoopArgs &A, int current, int n_cand, hipStream_t st);

// The loop fusion on the device (loop_fuse.hip): LoopClosing::searchAndFuse (loopClosing.cpp:496-516)
// with Matcher::fuseByPose (matcher.cpp:1135-1238) from the store, over section 4m's overlay and match list.  What
// vo_kfstore_enable_loop_fuse allocates, one block (C = max_corrected, P = max_loop_points): head [4] (passes of the last call,
// "the call runs" -- 0 when the _loop form met a compute_sim3 that is not ACCEPTED --, the length of its list, 0); base
// [C + 1], the call's match count at the start of a pass; rec [C][8]: (target, passed, matches, adds, replaces recorded,
// replaces that moved a carrier, cleared, undone) per pass; and `in`, the host form's arrays as its one copy brings them:
// S_corr [C][8] | corr_kf [C] | ids [P].
constexpr int kLfRecInts = 8;
enum { kLfTarget = 0, kLfPassed, kLfMatches, kLfAdds, kLfReplaces, kLfMoved, kLfCleared, kLfUndone };
enum { kLfPasses = 0, kLfRuns, kLfNPoints };
struct KfLoopFuseView {
  int C, P;
  int *head, *base, *rec;
  double *S_corr;
  int *corr_kf, *ids;
  size_t reset_bytes, in_bytes;  // from head: what a call resets; from S_corr: the whole of `in`
};

// The loop pose graph from the store (pose_graph_store.hip): the pose collection and the four edge
// families of Optimizer::solvePoseGraphLoop (optimizer_ceres.cpp:1062-1236) gathered on the device, and its write-back
// (:1264-1301).  What vo_kfstore_enable_pose_graph allocates, one block: ledge [max_kf][kPgMaxLoopEdges] ascending (-1 beyond
// n_ledge [max_kf]); node_of [max_kf] (node index or -1); cnt [max_corr + max_kf + 1], the edges of every family-A row and
// then of every key-frame, then their exclusive offsets; rl [max_kf][NK], the apply's refresh list (a point's id at its first
// live key, -1 elsewhere); swr [max_nodes][8]; `in`, a window's inputs packed by their counts (PgInputs); the WINDOW,
// contiguous so that one copy fetches it: rec, node_kf, quats, trans, scales, e_i, e_j, q_meas, t_meas, s_meas; and `sol`, a
// solver's quats | trans as the apply's one copy brings them.
constexpr int kPgRecInts = 16, kPgMaxLoopEdges = VO_KFSTORE_MAX_LOOP_EDGES, kPgMaxNodes = 4096 / 6 + 1, kPgMinWeight = 100;
enum { kPgNNodes = 0, kPgNEdges, kPgNA, kPgNB, kPgNC, kPgND, kPgStatus, kPgCurr, kPgMatch, kPgFixed, kPgNMoved, kPgNUnanchored };
struct KfPgView {
  int max_kf, NK, max_nodes, max_edges, max_corr, max_cp;
  int *ledge, *n_ledge, *node_of, *cnt, *rl;
  double *swr;
  uint8_t *in;
  size_t in_bytes;
  uint8_t *win;
  size_t win_bytes;
  int *rec, *node_kf;
  double *quats, *trans, *scales;
  int *e_i, *e_j;
  double *q_meas, *t_meas, *s_meas;
  uint8_t *sol;
  size_t sol_bytes;
};
// a window's inputs inside `in` (or a staging block laid out like it): S_corr | S_uncorr [n_corr][8], corr_kf [n_corr],
// lc_start [n_corr + 1], lc_kf [n_lc], cp_id | cp_ref [n_cp], every array rounded up to 16 bytes
struct PgInputs {
  int n_corr, n_lc, n_cp;
  double *S_corr, *S_unc;
  int *corr_kf, *lc_start, *lc_kf, *cp_id, *cp_ref;
  size_t bytes;
};

// The loop correction from the store (loop_correct.hip): the propagation of the loop Sim3 over the current
// key-frame's neighbours with the point correction (loopClosing.cpp:364-437) and the loop connections (:461-479).  What
// vo_kfstore_enable_loop_correct allocates, one block (C = max_corrected, P = max_corrected_points, E = max_loop_connections):
// rec [kLcRecInts] (enum below); cur [4], the one-entry list of step 1; scw [8], the loop Sim3 as the call received it; pos_of
// [max_kf], position + 1 in corr_kf (0: not corrected); perm [C], the list position of corr_kf[r]; S_inv [C][8], S_corr^-1; blk, the first-occurrence count of every workgroup of the index grid; cp_ent [P], the
// entry a corrected point is read at; rows [C][max_kf] bytes, a loop-connection row per list position; and the RESULT,
// contiguous so that one copy fetches it: list [C] (currConnect in list order), corr_kf [C], S_corr | S_unc [C][8], cp_id |
// cp_ref [P], lc_start [C + 1], lc_kf [E].
constexpr int kLcRecInts = 16;
enum { kLcNCorr = 0, kLcNCp, kLcNLc, kLcCurr, kLcStatus, kLcNRows, kLcConnStatus, kLcLive, kLcValid, kLcSetup };
struct KfLoopCorrectView {
  int C, P, E, max_kf, n_blk;
  int *rec, *cur;
  double *scw;
  int *pos_of, *perm;
  double *S_inv;
  int *blk, *cp_ent;
  uint8_t *rows;
  uint8_t *res;
  size_t res_bytes;
  int *list, *corr_kf;
  double *S_corr, *S_unc;
  int *cp_id, *cp_ref, *lc_start, *lc_kf;
};

// The merge of the loop matches from the store (loop_merge.hip): loopClosing.cpp:439-455, a step per
// feature of the current key-frame, on section 4m's overlay and fuse_ops.h.  What vo_kfstore_enable_loop_merge allocates, one
// block: head [4] (enum below); rec [kMgRecInts] (enum below); per feature of the current key-frame the step's PLAN -- branch
// [NK] (the branch taken, include/vo_hip.h's per_feature), kind [NK] (0 no step, kMgAlone, kMgOrdered), ordered [NK] (the
// ordered steps' features, ascending), node_entry / node_next [NK] (the overlay node of the add at that feature: the call walks
// the fusion layer's m_next / m_tail / a_head with THESE nodes, so that an add never meets max_candidates) -- which is what a
// call resets; and ids [NK], the host form's match_ids as its one copy brings them.
constexpr int kMgRecInts = 16;
enum { kMgRuns = 0, kMgCurr, kMgN, kMgNOrdered };  // head
enum { kMgSteps = 0, kMgAdds, kMgNoops, kMgReplaces, kMgMoved, kMgCleared, kMgDead, kMgUndone, kMgOrderedSteps, kMgRecCurr };
enum { kMgAlone = 1, kMgOrdered = 2 };
enum { kMgBrNone = 0, kMgBrAdd, kMgBrNoop, kMgBrReplace, kMgBrDead, kMgBrUndone };
struct KfLoopMergeView {
  int NK;
  int *head, *rec, *branch, *kind, *ordered, *node_entry, *node_next, *ids;
  size_t reset_bytes;  // from head: what a call resets
};

// Loop detection from the store (detect_loop.hip): LoopClosing::detectLoop (loopClosing.cpp:52-175) with
// its consistency groups, the erase locks of the loop thread (keyframe.cpp:541-557) and the composed loop-closing step.  What
// vo_kfstore_enable_detect_loop allocates, one block (D = max_detect_candidates, G = max_groups, words = ceil(max_kf / 64)):
// head [kDlHeadInts] (enum below: what carries over between calls -- the live half and its group count -- and what one call's
// kernels hand to each other, among it the three CSR pairs and the candidate count k_kfdb_query reads and writes); rec
// [kDlRecInts], the record (enum below); lrec [kDlLockInts], release_loop_locks' record: (n released, n pending, state, 0 |
// the pending key-frames); cand [D], the query's candidates; enough [D], enoughConCandidates_; counts [2][G], the groups'
// counters of either half; excl [max_kf], conn [max_kf], the query's lists; bits [2][G][words], the groups as bitsets over
// key-frames, ping-pong between the halves; cbits [D][words], the candidates' groups; consist [D][G] bytes.
constexpr int kDlHeadInts = 16, kDlRecInts = 16, kDlLockInts = 4 + VO_KFSTORE_LOOP_MAX_CANDIDATES + 4, kDlMaxGroups = VO_KFSTORE_DETECT_MAX_GROUPS;
enum { kDhRun = 0, kDhHalf, kDhNGroups, kDhNCand, kDhQStart, kDhExclStart = 6, kDhConnStart = 8, kDhMinScore = 10, kDhNEnough };
enum { kDlOutcome = 0, kDlCurrent, kDlNExcl, kDlNConn, kDlMinScore, kDlNCand, kDlGroupsBefore, kDlGroupsAfter, kDlNEnough, kDlLocked,
       kDlPending };
enum { kDkReleased = 0, kDkNPending, kDkState, kDkList = 4 };
struct KfDetectView {
  int D, G, max_kf, words;
  int *head, *rec, *lrec, *cand, *enough, *counts, *excl, *conn;
  unsigned long long *bits, *cbits;
  uint8_t *consist;
};
// compute_sim3 for a candidate list whose length only the device knows (loop_sim3.hip): the candidates are src[0 .. *dev_n) when
// *dev_go == go_value, else none; k_loop_begin_counted copies them into the block, sets their erase locks (loopClosing.cpp:208)
// and writes the count; the front and the construction are enqueued for max_candidates, and k_loop_trim puts the rows beyond
// the count back to what k_loop_begin left, so that everything a result reads is compute_sim3's for the same list.  No list
// (the sticky VO_KFSTORE_CONNECTIONS_INVALID) or more than max_candidates entries (the sticky VO_KFSTORE_LOOP_CAPACITY): nothing is
// walked and the state is NO MATCH with zero candidates (quiet: "no list" raises nothing -- the composed step, for which that is
// how almost every key-frame ends).  Launches and a memset only.
int loop_compute_counted(vo_kfstore *s, int current, const int *dev_go, int go_value, const int *dev_n, const int *dev_src, int fix_scale,
                         int n_rand, int32_t rand_max, int max_rounds, bool quiet = false);

// Key-frame creation on the device (keyframe_create.hip): VisualOdometry::createNewKeyFrame
// (visualOdometry.cpp:463-517) and the first key-frame of initVisualOdometry (:170-198) written into the store.  What
// vo_kfstore_enable_keyframe_create allocates, one block (P = pow2_ceil(NK)): keys [P], the depth walk's sort keys when they
// do not fit in LDS; created [NK] rows (feature, id) in walk order; rec [kKcRecInts]; stats [4], need_stats' counts of the host
// form; n_eff, the count the fill and k_featvec run with (n, or 0 when the frames form's n is not the slot's); and the step's
// scratch: slot [NK] (the slot's id after the temp cull, -1: null), first [NK] (the entry of that id's first observation),
// newid [NK] (the id of the point created at the feature, -1: none), word / node [NK] and weight [NK], k_bow_transform's
// outputs; `in`, the host forms' inputs as their one staging copy brings them: Tcw12 | x | y | octave | angle | depth |
// u_right | slot ids [NK] each | desc [NK][32].
constexpr int kKcRecInts = 16, kKcLdsKeys = 4096;
enum { kKcKeyframe = 0, kKcN, kKcNPairs, kKcNWalked, kKcNCreated, kKcNTracked, kKcFirstId, kKcNextId, kKcEarly, kKcStatus };
struct KfCreateView {
  int NK, P;
  unsigned long long *keys;
  int2 *created;
  int *rec, *stats, *n_eff, *slot, *first, *newid, *word, *node;
  double *weight;
  uint8_t *in;
  size_t in_bytes;
};
// where the columns of a host form lie inside `in` (or a staging block laid out like it)
struct KcInputs {
  double *T;
  float *x, *y, *angle, *depth, *u_right;
  int *octave, *slot;
  uint8_t *desc;
};
__host__ __device__ __forceinline__ KcInputs kc_inputs(uint8_t *in, int NK) {
  const size_t col = ((size_t)NK * 4 + 15) & ~(size_t)15;
  KcInputs I;
  I.T = reinterpret_cast<double *>(in);
  uint8_t *p = in + 96;
  I.x = reinterpret_cast<float *>(p), I.y = reinterpret_cast<float *>(p + col), I.octave = reinterpret_cast<int *>(p + 2 * col);
  I.angle = reinterpret_cast<float *>(p + 3 * col), I.depth = reinterpret_cast<float *>(p + 4 * col);
  I.u_right = reinterpret_cast<float *>(p + 5 * col), I.slot = reinterpret_cast<int *>(p + 6 * col), I.desc = p + 7 * col;
  return I;
}

// pair p = f * per + c searches key-frame dev_pair_kf[p] of the store (a number outside [0, size): no key-frame, the pair
// matches nothing); per <= the buffers' `per`.  search_bad: a key-frame flagged bad is searched like any other
// (trackRefKeyFrame) instead of matching nothing (relocalisation).
int bow_walk_replay(vo_frames *frames, int B, int per, const KfStoreView &S, const int *dev_pair_kf, float ratio, int check_rot,
                    BowWalkBufs &b, int32_t *dev_assigned, int32_t *dev_n_matches, hipStream_t st, hipEvent_t ev0 = nullptr,
                    hipEvent_t ev1 = nullptr, bool search_bad = false);  // (events around k_bow_walk)

// vo_tracker_build_local_map's kernels (local_map.hip): votes, voters, expansion (k_lm_keyframes, a workgroup per frame),
// the local points (k_lm_points, a workgroup per frame).  Enqueued on st; the caller orders st against the store's stream.
struct LocalMapArgs {
  KfStoreView S;
  KfObsView O;
  int B, cap, max_local, stride;  // frames, feature slots per frame, local points per frame, row stride of the local-map arrays
  const int *fn;                  // [B] features per frame
  const int *winner;              // [B] < 0: the frame's relocalisation failed (NULL: every frame takes part)
  int *sid;                       // [B][cap] slot ids (relocalisation), or NULL: read through ref_kf / assigned
  const int *ref_kf, *assigned;   // [B], [B][cap] the reference-key-frame route's key-frame numbers and first-search matches
  uint8_t *fhas, *fobs;           // [B][cap]
  int *votes;                     // [B][S.max_kf] scratch: the counts, then list position + 1 per key-frame
  int *lkf, *n_kf, *best, *n_pts; // [B][VO_TRACKER_LOCAL_MAX_KEYFRAMES], [B], [B], [B]
  int *err;                       // the store routes' sticky word
  double *p1, *nrm1;
  float *mind1, *maxd1;
  uint8_t *pf1, *desc1;
  int *link1, *ids1;
};
int local_map_build(const LocalMapArgs &A, hipStream_t st);

// ---- the opt-in layers of a store, one bit each in vo_kfstore::layers.  Every vo_kfstore_enable_* starts with
// enable_begin, every other entry point of a layer with need (kfstore.hip).
enum KfLayer : unsigned {
  kLayerConnections = 1u << 0,
  kLayerCulling = 1u << 1,
  kLayerMapping = 1u << 2,
  kLayerLocalBa = 1u << 3,
  kLayerUpkeep = 1u << 4,
  kLayerFuse = 1u << 5,
  kLayerLoop = 1u << 6,
  kLayerPoseGraph = 1u << 7,
  kLayerKeyframeCreate = 1u << 8,
  kLayerLoopFuse = 1u << 9,
  kLayerLoopCorrect = 1u << 10,
  kLayerLoopMerge = 1u << 11,
  kLayerDetectLoop = 1u << 12,
};

// The window protocol local BA and the pose graph share: a *_window call enqueues the window and notes the store's
// generation (begin); fetch brings it down in ONE copy into the staging block and caches its record (the first 16 ints of
// both windows, status at kBaStatus == kPgStatus); an *_apply is valid for the window of the store's current generation only.
static_assert(kBaRecInts == 16 && kPgRecInts == 16 && (int)kBaStatus == (int)kPgStatus, "KfWindow holds either window's record");
struct KfWindow {
  OwnedPinnedBuf stage;  // the window coming down, or a window's inputs / a solver's result going up: one copy each
  bool enqueued = false, rec_known = false;  // a window has been enqueued; its record has been fetched
  unsigned long long gen = 0;                // the store's generation when it was
  int32_t rec[16] = {0};
  void begin(unsigned long long store_gen) { enqueued = true, rec_known = false, gen = store_gen; }
  int fetch(const uint8_t *dev_win, size_t win_bytes, bool record_only, hipStream_t st, const char *W);
  // the host address of a window array inside the staging block
  template <class T>
  T *staged(const T *dev_ptr, const uint8_t *dev_win) const {
    return reinterpret_cast<T *>(stage.data() + (reinterpret_cast<const uint8_t *>(dev_ptr) - dev_win));
  }
  // the guards of an *_apply: a window of this generation (its record fetched when not yet known) whose status is OK
  int check_apply(const char *W, unsigned long long store_gen, const uint8_t *dev_win, hipStream_t st);
};

}  // namespace vo

struct vo_kfstore {
  int max_kf = 0, NK = 0, size = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  vo::KfStoreView V{};
  vo::OwnedDevBuf rec;
  vo::OwnedPinnedBuf stage;
  std::vector<int> n;  // features per key-frame (host copy: update_points' lengths)
  // what vo_tracker_build_local_map reads beyond the records (KfObsView)
  vo::OwnedDevBuf graph, normals, okeys, orun;
  int okeys_cap = 0;      // keys the index holds: the power of two above max_kf * NK, at least one chunk
  bool obs_dirty = true;  // an insert or update_points has happened since the index was built
  int obs_n = 0;          // keys the built index spans (a power of two covering size * NK)
  unsigned layers = 0;    // the vo::KfLayer bits of the layers enabled on this store
  // the generation word: every call that writes the store advances it; an apply is valid for the window of its generation
  unsigned long long gen = 0;
  vo::KfConnections *conn = nullptr;  // vo_kfstore_enable_connections: the graph is then maintained on the device (section 4h)
  vo::OwnedDevBuf cull;               // vo_kfstore_enable_culling: the columns and words of section 4i
  vo::KfCullView X{};
  vo::OwnedDevBuf map;                // vo_kfstore_enable_mapping: the arrays of section 4j
  vo::KfMapView M{};
  size_t map_bytes = 0;
  vo::OwnedDevBuf ba;                 // vo_kfstore_enable_local_ba: the arrays of section 4k
  vo::KfBaView B{};
  vo::KfWindow ba_win;
  std::vector<double> ba_poses, ba_points;  // the composed call's solver state (sized by the capacities: no allocation per call)
  std::vector<uint8_t> ba_erase;
  vo::OwnedDevBuf up;                 // vo_kfstore_enable_point_upkeep: the block of section 4l
  vo::OwnedPinnedBuf up_stage;        // a host form's lists going up: one copy
  vo::KfUpkeepView U{};
  vo::OwnedDevBuf fu;                 // vo_kfstore_enable_fuse: the block of section 4m
  vo::KfFuseView F{};
  vo::OwnedDevBuf lp;                 // vo_kfstore_enable_loop: the block of section 4n
  vo::OwnedPinnedBuf lp_stage;        // a host form's candidates and rand() values going up, the results coming down: one copy each
  vo::KfLoopView L{};
  bool loop_called = false;
  int loop_fix_scale = 1;             // of the last compute_sim3: what compute_sim3_continue refines with
  vo::OwnedDevBuf pg;                 // vo_kfstore_enable_pose_graph: the block of section 4o
  vo::KfPgView P{};
  vo::KfWindow pg_win;
  int pg_counts[3] = {0, 0, 0};       // n_corr, n_lc, n_cp of the last window: where its inputs lie in P.in
  std::vector<int32_t> pg_ledge;      // the loop edges as the host knows them: [max_kf][1 + VO_KFSTORE_MAX_LOOP_EDGES], count first
  std::vector<double> pg_q, pg_t;     // the composed call's solver state (sized by the capacities: no allocation per call)
  vo::OwnedDevBuf kc;                 // vo_kfstore_enable_keyframe_create: the block of section 4p
  vo::OwnedPinnedBuf kc_stage;        // a host form's inputs going up: one copy
  vo::KfCreateView K{};
  vo::OwnedDevBuf lf;                 // vo_kfstore_enable_loop_fuse: the block of section 4q
  vo::OwnedPinnedBuf lf_stage;        // the host form's arrays going up, the result coming down: one copy each
  vo::KfLoopFuseView Q{};
  vo::OwnedDevBuf lc;                 // vo_kfstore_enable_loop_correct: the block of section 4r
  vo::OwnedPinnedBuf lc_stage;        // the host form's Sim3 going up, the result coming down: one copy each
  vo::KfLoopCorrectView R{};
  vo::OwnedDevBuf lm;                 // vo_kfstore_enable_loop_merge: the block of section 4s
  vo::OwnedPinnedBuf lm_stage;        // the host form's match_ids going up, the result coming down: one copy each
  vo::KfLoopMergeView G{};
  vo::OwnedDevBuf dl;                 // vo_kfstore_enable_detect_loop: the block of section 4t
  vo::OwnedPinnedBuf dl_stage;        // a result coming down, the composed step's one read
  vo::KfDetectView Dv{};
  int dl_current = -1;                // `current` of the last detect_loop (-1: none yet): what compute_sim3_detected walks for
  int last_loop_kf = 0;               // lastLoopKFId_ (loopClosing.cpp:13, :491) of the composed step
  uint8_t *record(int k) const { return rec.as<uint8_t>() + (size_t)k * V.rec; }
};

namespace vo {

// VO_OK when every bit of `layers` is enabled on s; else VO_ERR_INVALID, with "<W>: vo_kfstore_enable_<layer> has not been
// called on this store" for the first missing one (no message when s is NULL)
int need(const vo_kfstore *s, const char *W, unsigned layers);
int need_keyframe(const vo_kfstore *s, const char *W, int keyframe);
// The common head of every vo_kfstore_enable_*, in the order the calls have always answered in: `required` missing ->
// VO_ERR_INVALID; !args_ok -> VO_ERR_INVALID; a store that holds key-frames -> VO_ERR_INVALID; `layer` enabled already ->
// kLayerEnabled (the caller returns VO_OK with nothing done); else VO_OK, and the caller allocates and sets the bit.
constexpr int kLayerEnabled = 1;
int enable_begin(const vo_kfstore *s, const char *W, unsigned required, unsigned layer, bool args_ok = true);

}  // namespace vo
