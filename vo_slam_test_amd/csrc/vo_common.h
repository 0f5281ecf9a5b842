// vo_common.h -- shared host/device helpers for the gfx950 library (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include <vector>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vo_hip.h"

namespace vo {

void set_error(const char *fmt, ...);
int ensure_device();  // VO_OK or VO_ERR_NO_DEVICE

#define VO_HIP_CHECK(expr)                                                                 \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      vo::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return VO_ERR_HIP;                                                                   \
    }                                                                                      \
  } while (0)

#define VO_CHECK(expr)           \
  do {                           \
    int _s = (expr);             \
    if (_s != VO_OK) return _s;  \
  } while (0)

// growable device buffer
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  bool view = false;  // p points into another DevBuf (an arena): never freed through this object
  int reserve(size_t n) {
    if (view) p = nullptr, bytes = 0, view = false;
    if (n <= bytes) return VO_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    VO_HIP_CHECK(hipMalloc(&p, n));
    bytes = n;
    return VO_OK;
  }
  void release() {
    if (p && !view) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    view = false;
  }
  void set_view(void *ptr, size_t n) {  // (an owned allocation is kept aside by the caller or released first)
    if (p && !view) (void)hipFree(p);
    p = ptr, bytes = n, view = true;
  }
  template <class T>
  T *as() const {
    return reinterpret_cast<T *>(p);
  }
};

// Grow-only device scratch of the stateless entry points: one set per host thread (`thread_local ScratchBuf`), kept
// between calls so that the hot path neither allocates nor frees (hipFree synchronises the whole device).  Every
// ScratchBuf registers itself with its thread; vo_release_thread_scratch() frees what the calling thread holds (the
// buffers grow again on the next call), e.g. before a worker thread exits or after a one-off 150 MB pose graph.
struct ScratchBuf : DevBuf {
  ScratchBuf();
};
size_t release_thread_scratch();  // bytes freed

// Grow-only page-locked host staging (per host thread where used): copies to and from it run at full PCIe
// rate and without the runtime's own bounce buffer.  Never freed (thread-exit order vs. runtime teardown).
struct PinnedBuf {
  void *p = nullptr;
  size_t bytes = 0;
  int reserve(size_t n) {
    if (n <= bytes) return VO_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    const size_t want = n + n / 2 + 4096;
    VO_HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
    bytes = want;
    return VO_OK;
  }
  uint8_t *data() const { return reinterpret_cast<uint8_t *>(p); }
};

// ---- memory of a handle: freed when the handle is deleted, after its streams have drained.  The
// types above stay as they are for per-thread and static scratch, which is never freed.
struct OwnedDevBuf : DevBuf {
  OwnedDevBuf() = default;
  OwnedDevBuf(const OwnedDevBuf &) = delete;
  OwnedDevBuf &operator=(const OwnedDevBuf &) = delete;
  ~OwnedDevBuf() { release(); }
};
struct OwnedPinnedBuf : PinnedBuf {
  OwnedPinnedBuf() = default;
  OwnedPinnedBuf(const OwnedPinnedBuf &) = delete;
  OwnedPinnedBuf &operator=(const OwnedPinnedBuf &) = delete;
  ~OwnedPinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};

// One device block for a set of arrays whose sizes are fixed when the set is created.  A layout function names every
// array once -- take(field of the handle's view struct, bytes) -- and build() runs it twice: the first pass measures, one
// hipMalloc follows, the second pass hands out the addresses.  Every array starts on a 4 KiB boundary (no less aligned
// than an allocation of its own); its byte count, slack included, is the caller's.
struct Arena {
  uint8_t *block = nullptr;
  size_t bytes = 0, at = 0;
  Arena() = default;
  Arena(const Arena &) = delete;
  Arena &operator=(const Arena &) = delete;
  ~Arena() {
    if (block) (void)hipFree(block);
  }
  template <class T>
  void take(T *&field, size_t n) {
    field = block ? reinterpret_cast<T *>(block + at) : nullptr;
    at += (n + 4095) & ~(size_t)4095;
  }
  template <class Layout>
  int build(Layout &&layout, const char *what) {
    if (block) (void)hipFree(block);  // (a set laid out again, e.g. after a failed first attempt)
    block = nullptr, at = 0, layout(*this);
    const size_t need = at;
    VO_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&block), need ? need : 4096));
    bytes = need, at = 0, layout(*this);
    if (at != need) {  // the two passes disagree: an array would overlap its neighbour
      set_error("%s: the array layout measured %zu bytes and assigned %zu", what, need, at);
      return VO_ERR_HIP;
    }
    return VO_OK;
  }
};

constexpr int kWave = 64;

// Per host thread: a non-blocking stream for the stateless entry points (vo_hamming_matrix, vo_pose_only_solve,
// vo_sim3_solve, vo_pose_graph_solve, ...).  The reference calls them concurrently from the tracking, local-
// mapping and loop-closing threads: on the legacy NULL stream a 0.4 ms pose-only solve would queue behind a
// 500-key-frame pose graph, and every hipDeviceSynchronize would stall the other threads' streams.  Created on
// first use, never destroyed (thread-exit order vs. runtime teardown).
hipStream_t thread_stream();
// checked copies on a stream (error text names `what`)
int copy_h2d(void *dst, const void *src, size_t bytes, hipStream_t st, const char *what);
int copy_d2h(void *dst, const void *src, size_t bytes, hipStream_t st, const char *what);
int stream_sync(hipStream_t st, const char *what);
// reserve + copy
int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t st, const char *what);

// Dense SPD solve on the device (csrc/chol.hip).  A: (ld + 64) rows x ld columns, row-major, ld a multiple of 64.
// Rows 0..ld-1: the matrix, lower triangle used (identity on the padding diagonal); row ld: the right-hand side;
// rows ld+1.. are spare.  The lower triangle is factored in place (L L^T, 64 x 64 tiles, one persistent dataflow
// kernel on the FP64 matrix cores); the solution ends up in row ld + 1.  `workspace`: chol_workspace_bytes(ld) bytes
// of device memory; its first int is the fail flag -- zeroed by the caller, set to 1 when a pivot is not positive,
// 2 when the kernel abandoned a wait.  Enqueues one memset and one kernel; no synchronisation.
constexpr int kCholPanel = 64;
size_t chol_workspace_bytes(int ld);
// `plan` (or NULL = dense): the tile structure of the matrix.  chol_plan_create(m, pattern): m = ld / 64 tile rows, bit k of
// pattern[i] = tile (i, k) of the lower triangle may be non-zero (the fill of the factorisation is added by the symbolic
// pass); tiles outside the plan are never read, written or waited for, and tile columns that do not depend on each
// other are factored concurrently.  chol_symbolic is that pass on its own (for choosing an ordering on the host).
struct CholPlan;
CholPlan *chol_plan_create(int m, const unsigned long long *pattern);
void chol_plan_destroy(CholPlan *p);
void chol_plan_info(const CholPlan *p, int *n_tiles, int *depth, int *n_updates = nullptr);
void chol_symbolic(int m, const unsigned long long *pattern, unsigned long long *lmask, int *depth, int *n_tiles);
void chol_factor_solve(double *A, int ld, void *workspace, hipStream_t st, const CholPlan *plan = nullptr);
// Split solve over the ranks of a sharded system (chol.hip): the segments of a nested-dissection order occupy the tile
// columns [0, c0), the separators [c0, m); `own` = this rank's segment columns.  Phase 1 eliminates them into the separator
// block, phase 2 solves the (rank-summed) separator block, phase 3 substitutes back into the rank's segments.
CholPlan *chol_plan_create_split(int m, const unsigned long long *pattern, int c0, unsigned long long own, int phase);
void chol_split_phase(double *A, int ld, void *workspace, hipStream_t st, const CholPlan *plan, int phase, int c0);
// Order of the nf diagonal blocks (bs rows each; pairs = the off-diagonal blocks (hi, lo) that are non-zero) of a system
// with m tile rows: natural, or a nested dissection of a (cyclic) band when that shortens the chain of dependent tile
// columns by a quarter or more (chol.hip).  force_parts: -1 = choose, 1 = natural, P > 1 = P segments.
struct CholOrder {
  std::vector<int> slot_of;  // natural block index -> position
  int parts = 1, cyclic = 0, sep = 0, depth = 0, tiles = 0;
  std::vector<unsigned long long> pattern;  // tile pattern in the chosen order (chol_plan_create's input)
  std::vector<int> part_of;  // position -> segment index, -1 = separator (empty: natural order, no segments)
  int seg_slots = 0;         // positions [0, seg_slots) are the segments', the rest the separators'
};
CholOrder chol_choose_order(int nf, int bs, const std::vector<std::pair<int, int>> &pairs, int m, int force_parts = -1);

// searchByBoW(KeyFrame*, Frame*) (matcher.cpp:449-559) for B (reference key-frame, current frame) pairs whose current
// frames are resident in a frame store (slots slot0 .. slot0 + B - 1): Frame::computeBow (vocabulary transform, levelsup)
// on the device, the common-node walk on the host (this call synchronises `st` once), one k_node_replay launch with a
// workgroup per pair reading the frames' descriptors and angles in place.  dev_assigned [B][cap]: key-frame feature index
// held by each frame feature or -1; dev_n_matches [B].  (match.hip; the key-frame side is host memory.)
struct RefKeyFrame {
  int n;
  const uint8_t *valid;  // [n] the feature's map point exists and is not bad
  const uint8_t *desc;   // [n][32]
  const float *angle;    // [n]
  const vo_bow_view *nodes;
};
// `per` key-frames per frame (relocalisation candidates): kfs [B * per], pair p = f * per + c searches slot slot0 + f and
// owns dev_assigned [p][cap], dev_n_matches [p]; a pair with n == 0 matches nothing.  With `own` the call works in the
// caller's buffers instead of the calling thread's and does NOT synchronise at its end: the caller must not call again
// before the stream has drained (the synchronisation up front does that for calls on the same stream).
struct BowResidentBufs {  // (a handle's: the calling thread's own set is bow_search_resident's)
  OwnedDevBuf w, wt, node, img;
  OwnedPinnedBuf stage, up;
};
int bow_search_resident(const vo_vocab *v, vo_frames *frames, int slot0, int B, const RefKeyFrame *kfs, float ratio, int check_rot,
                        int levelsup, int32_t *dev_assigned, int cap, int32_t *dev_n_matches, hipStream_t st, int per = 1,
                        BowResidentBufs *own = nullptr);
// vo_vocab_train's use of the tree it has built (match.hip): k_bow_transform over resident descriptors (4-byte aligned) into
// resident outputs, enqueued on st; the node weights replaced (synchronises st)
int vocab_transform_resident(const vo_vocab *v, int n, const uint32_t *dev_desc, int levelsup, int *dev_word, double *dev_weight,
                             int *dev_node, hipStream_t st);
int vocab_set_weights(vo_vocab *v, const double *node_weight, hipStream_t st);
// device views of a frame store's per-slot arrays (guided.hip)
struct FrameStoreView {
  int cap;
  const uint8_t *desc;  // [slots][cap][32]
  const float *angle;   // [slots][cap]
  const int *n;         // [slots]
  const float *x = nullptr, *y = nullptr, *uright = nullptr;  // [slots][cap]
  const int *octave = nullptr;
};
FrameStoreView frame_store_view(const vo_frames *h);

// The relocalisation route of the tracker (reloc.hip): VisualOdometry::relocalization() (visualOdometry.cpp:313-395) for
// the frames resident in the tracker's frame store.  The tracker owns the per-feature frame state and the pose solver's
// buffers (RelocShared); the candidates, the PnP problems and the per-frame walk state live in the Reloc object.
struct Reloc;
struct RelocShared {
  vo_frames *frames;
  const vo_vocab *vocab;
  int B, cap, n_levels, width, height;
  const float *sf;      // host, n_levels
  float cam5[5];
  const double *cam5d;  // device
  double *pose;         // [B][6]
  double *fpoint;       // [B][cap][3]
  uint8_t *fhas, *foutl;
  uint8_t *fobs;        // [B][cap] the slot's map point has observations
  double *pts, *obs, *isg;
  int *ranges, *index;
  uint8_t *outlier;
  int *ninl, *assigned, *nm;
  uint8_t *resblk;
  const int *orb_err, *guided_err;
  hipStream_t st;
};
int reloc_create(Reloc **out, int B, int cap, int max_cand, int max_feat, const float *sf, int n_levels);
void reloc_destroy(Reloc *r);
int reloc_set_candidates(Reloc *r, const vo_vocab *vocab, int max_cand, const int32_t *n_cand, const vo_reloc_candidate *cands,
                         hipStream_t st);
int reloc_run(Reloc *r, const RelocShared &S);
// trackLocalMap behind a relocalisation (vo_tracker_track_local_map after vo_tracker_relocalize*).  reloc_local_prep: the
// local points whose id the frame already holds lose their flags (q1_flags = the flags Frame::isInFrame is then run with),
// `assigned` is cleared, *frame_on [B] = the per-frame query count of the steps in between (-1: the frame's relocalisation
// failed, it is left out).  The caller runs isInFrame and the search; reloc_local_finish writes the matches into the slots,
// solves over all non-null slots and writes the counts and the frames' records of the result block.
struct RelocLocalArgs {
  int nq, stride;
  const uint8_t *pf1;
  uint8_t *q1_flags;
  const int *ids1;  // or NULL: nothing is skipped
  const double *p1;
};
int reloc_local_prep(Reloc *r, const RelocShared &S, const RelocLocalArgs &L, const int **frame_on);
int reloc_local_finish(Reloc *r, const RelocShared &S, const RelocLocalArgs &L);
// device array behind a VO_TRACKER_RELOC_* selector (nullptr: not one of them)
const void *reloc_selector(const Reloc *r, int what, size_t *bytes);

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
// allocated once by connections_create (connections_bytes(max_kf) bytes; `graph`: the store's graph rows, which the calls
// rewrite); connections_reserve sizes the scratch of a list of n entries (grow-only) and returns the device list of the
// host form; connections_update enqueues three launches on st and nothing else.
struct KfConnections;
size_t connections_bytes(int max_kf);
int connections_create(KfConnections **out, int max_kf, int *graph, hipStream_t st);
void connections_destroy(KfConnections *c);
int connections_reserve(KfConnections *c, int n, int **dev_list);
int connections_update(KfConnections *c, const KfStoreView &S, const KfObsView &O, int n, const int *dev_list, hipStream_t st);
int connections_status(KfConnections *c, hipStream_t st, int *word);  // synchronises; bit 0: invalid number, bit 1: children
int connections_get(KfConnections *c, int size, int k, hipStream_t st, int32_t *n_connected, int32_t *weights, int32_t *n_ordered,
                    int32_t *ordered, int32_t *ordered_weights, int32_t *parent, int32_t *n_children, int32_t *children);
// for the culling kernels (cull.hip): the state's arrays; the `erased` column every later update and ordering pass
// honours (NULL until vo_kfstore_enable_culling); k_conn_order over the touched key-frames on its own (one launch)
struct KfConnView {
  int max_kf;
  int *W, *ordered, *n_ordered, *mode, *parent, *touched, *status;
};
KfConnView connections_view(const KfConnections *c);
void connections_set_erased(KfConnections *c, const int *erased);
int connections_order(KfConnections *c, int size, hipStream_t st);

// Key-frame culling on the device (cull.hip): LocalMapping::cullingKeyFrames with
// KeyFrame::eraseKeyFrame, eraseConnection and MapPoint::eraseObservedKF.  cols: [max_kf][3][NK] -- octave (int32), depth,
// u_right (float) of a key-frame side by side, so that the host form of set_keypoints is one copy; erased, locked, pending
// [max_kf]; rec [max_kf] (key-frame, mp_cnt, re_obs, decision) of the last cull call and n_rec its candidate count.
// cull_bytes is what cull_layout hands out of one block; cull_init writes the defaults; cull_enqueue is k_cull_count +
// k_cull_apply, erase_enqueue the erase alone, both without the ordering pass.  Launches only.
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
size_t cull_bytes(int max_kf, int NK);
KfCullView cull_layout(void *block, int max_kf, int NK);
int cull_init(const KfCullView &X, int max_kf, hipStream_t st);
int cull_set_lock(const KfCullView &X, int k, int on, hipStream_t st);
int cull_enqueue(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, int current, float th_depth,
                 hipStream_t st);
int erase_enqueue(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, int keyframe, hipStream_t st);

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
size_t mapping_bytes(int max_kf, int NK);
KfMapView mapping_layout(void *block, int max_kf, int NK);
int mapping_init(const KfMapView &M, size_t bytes, int first_point_id, hipStream_t st);
int mapping_set_pose_dev(const KfMapView &M, int k, const double *dev_Tcw12, hipStream_t st);
int mapping_split_xy(const KfMapView &M, int k, int n, const float *dev_xy, hipStream_t st);
// one neighbour step = three launches.  tri_walk_replay (match.hip): k_tri_walk -- the step's neighbour from `current`'s
// graph row, its status and geometry (new_points_geom.h), the record's entry (the whole record on step 0), the store-to-
// store common-node walk and the argument block -- then k_node_replay in triangulation mode; `status`: the store's sticky
// word.  np_create (new_points.hip): k_np_create.
size_t tri_args_bytes();
int tri_walk_replay(const KfStoreView &S, const KfCullView &X, const KfMapView &M, const int *graph, int *status, int current, int step,
                    hipStream_t st);
// (ref_kf: the column of a store with local BA, else NULL -- a created point's keyFrame_ref_ is `current`, mappoint.cpp:37)
int np_create(const KfStoreView &S, const KfCullView &X, const KfMapView &M, double *normals, int *ref_kf, int current, int step,
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
size_t ba_store_bytes(int max_kf, int NK, int max_cams, int max_points, int max_edges);
KfBaView ba_store_layout(void *block, int max_kf, int NK, int max_cams, int max_points, int max_edges);
int ba_store_init(const KfBaView &B, int max_kf, hipStream_t st);
// five launches: local cameras, first-occurrence counts, points (with their edge counts and the fixed marks), layout (fixed
// cameras, capacities, poses, edge offsets), edges
int ba_window_enqueue(const KfStoreView &S, const KfObsView &O, const KfConnView &C, const KfCullView &X, const KfMapView &M,
                      const KfBaView &B, int current, hipStream_t st);
// two launches on the inputs in B.in: erase + death (and the poses), then write + refresh
int ba_apply_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                     double *normals, int *status, int n_cams, int n_points, int n_edges, hipStream_t st);
// the refresh alone for the n ids in B.ids_in
int ba_refresh_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                       double *normals, int *status, int n, hipStream_t st);
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
size_t upkeep_bytes(int max_recent, int NK);
KfUpkeepView upkeep_layout(void *block, int max_recent, int NK);
int upkeep_init(const KfUpkeepView &U, hipStream_t st);
// computeDescriptor for the n entries of a device list (negative: skipped): a memset of the overflow count and two launches
int upkeep_descriptors_enqueue(const KfStoreView &S, const KfObsView &O, const KfUpkeepView &U, int *status, int n, const int *dev_ids,
                               hipStream_t st);
// processNewKeyFrame up to the connection update: classify (U.list = the tracked ids, U.cand = the ids to append, per feature
// of `current`), refresh, descriptors, append
int upkeep_process_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                           const KfUpkeepView &U, double *normals, int *status, int current, hipStream_t st);
int upkeep_created_enqueue(const KfMapView &M, const KfUpkeepView &U, int *status, int current, hipStream_t st);
int upkeep_stats_enqueue(const KfUpkeepView &U, int n, const int *dev_ids, const int *dev_visible, const int *dev_found, hipStream_t st);
int upkeep_cull_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfUpkeepView &U, int current, hipStream_t st);

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
size_t fuse_bytes(int NK, int max_matches, int n_slots);
KfFuseView fuse_layout(void *block, int NK, int max_matches, int n_slots, const float bounds[4]);
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
// one fuse call on its own: reset, then mark / search / mutate for step 0 over the n ids of a device list
int fuse_single_enqueue(const FuseArgs &A, int target, int n, const int *dev_ids, float threshold, hipStream_t st);
// the composed call up to the closing rebuild: reset, target list and snapshot, 60 target steps, the gather, the closing step
int fuse_neighbors_enqueue(const FuseArgs &A, int current, hipStream_t st);
// current's live ids, each once, into F.snap (behind the rebuild: the list of the closing descriptors and refresh)
int fuse_live_list_enqueue(const FuseArgs &A, int current, hipStream_t st);

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
size_t loop_bytes(int NK, int max_cand, int max_pts, int max_rand, int n_slots);
KfLoopView loop_layout(void *block, int NK, int max_cand, int max_pts, int max_rand, int n_slots);
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
// the tables and constants of the block, once (ransacMaxIters by N from the host's libm; the camera as doubles)
int loop_init(const KfLoopView &L, const KfMapView &M, size_t bytes, hipStream_t st);
// a new call: the state reset, `current` checked, the front (match.hip: loop_bow_replay) and the solvers' construction
int loop_begin_enqueue(const LoopArgs &A, int current, int n_cand, int fix_scale, int n_rand, int rand_max, hipStream_t st);
// `rounds` rounds (walk to the next verification or to the end, then verify), then the steps behind a match; launches only
int loop_rounds_enqueue(const LoopArgs &A, int rounds, int fix_scale, hipStream_t st);
// the front's searchByBoW(current, cand[c], mode 1, checkRot) for c < n_cand in ONE k_node_replay launch (match.hip)
int loop_bow_replay(const LoopArgs &A, int current, int n_cand, hipStream_t st);
// k_sim3 (sim3.hip) on device-resident inputs: problem p owns off[p] .. off[p + 1]; nothing is copied or synchronised
int sim3_solve_dev(int n_problems, int fix_scale, const int *off, const double *Pm, const double *pxc, const double *isc, const double *Pc,
                   const double *pxm, const double *ism, const double *cam4, double *poses, double *scales, uint8_t *outlier, int *n_inliers,
                   vo_lm_summary *sums, hipStream_t st);

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
PgInputs pg_inputs(void *block, int n_corr, int n_lc, int n_cp);
size_t pg_store_bytes(int max_kf, int NK, int max_edges, int max_corr, int max_cp);
KfPgView pg_store_layout(void *block, int max_kf, int NK, int max_edges, int max_corr, int max_cp);
int pg_store_init(const KfPgView &P, hipStream_t st);
// addLoopEdge both ways and both erase locks; one launch
int pg_add_loop_edge(const KfPgView &P, const KfCullView &X, int a, int b, hipStream_t st);
// four launches: nodes (with the inputs' checks and the node Sim3s), counts, layout, emit
int pg_window_enqueue(const KfStoreView &S, const KfConnView &C, const KfCullView &X, const KfMapView &M, const KfPgView &P,
                      const PgInputs &I, int curr, int match, hipStream_t st);
// two launches on the solver's result in P.sol: poses and S_wr, then the re-anchoring with the refresh list
int pg_apply_enqueue(const KfStoreView &S, const KfObsView &O, const KfCullView &X, const KfMapView &M, const KfBaView &B,
                     const KfPgView &P, const PgInputs &I, int n_nodes, hipStream_t st);

// vo_kfdb_query_reloc_dev on a stream of the caller's (kfdb.hip): the database's own stream and `st` are ordered around the
// query by events.  Nothing is validated beyond what vo_kfdb_query_reloc_dev checks.
void kfdb_info(const vo_kfdb *db, int *size, int *max_batch);
int kfdb_query_reloc_on(vo_kfdb *db, hipStream_t st, int n_queries, const int32_t *q_start, const int32_t *q_words,
                        const double *q_values, const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand);

// ---- searchByBoW against key-frames of a store with the common-node walk on the device (match.hip): k_bow_transform and
// k_featvec build every resident frame's FeatureVector; k_bow_walk writes every (frame, candidate) pair's query list and
// argument block; k_node_replay runs as in bow_search_resident.  All buffers are sized once from (B, cap, per, NK).  A
// tracker owns ONE set, shared by its store routes: relocalisation walks `per` candidates per frame, trackRefKeyFrame one.
struct BowWalkBufs {
  int B = 0, cap = 0, per = 0, NK = 0;
  Arena mem;
  int *w, *node, *fv_nn, *fv_node, *fv_start, *fv_feat;  // [B][cap] word and node of every feature slot; the frames' FeatureVectors:
  double *wt;                                            // [B], [B][cap], [B][cap + 1], [B][cap]; [B][cap] weight
  int4 *queries, *claims;                                // [B * per][NK] each
  uint8_t *args, *ones;                                  // [B * per] argument blocks (match.hip's NodeArgs), [cap] ones
};
int bow_walk_reserve(BowWalkBufs &b, int B, int cap, int per, int NK, hipStream_t st);
int bow_featvec_resident(const vo_vocab *v, vo_frames *frames, int B, int levelsup, BowWalkBufs &b, hipStream_t st,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);  // (events around k_featvec)
// pair p = f * per + c searches key-frame dev_pair_kf[p] of the store (a number outside [0, size): no key-frame, the pair
// matches nothing); per <= the buffers' `per`.  search_bad: a key-frame flagged bad is searched like any other
// (trackRefKeyFrame) instead of matching nothing (relocalisation).
int bow_walk_replay(vo_frames *frames, int B, int per, const KfStoreView &S, const int *dev_pair_kf, float ratio, int check_rot,
                    BowWalkBufs &b, int32_t *dev_assigned, int32_t *dev_n_matches, hipStream_t st, hipEvent_t ev0 = nullptr,
                    hipEvent_t ev1 = nullptr, bool search_bad = false);  // (events around k_bow_walk)
// the FeatureVector of n features from their node ids (device arrays): n_nodes into *dev_n_nodes, node [n] ascending,
// start [n + 1], feat [n] (the features of a node in index order); n <= 16384
int featvec_dev(int n, const int *dev_node_of_feature, int *dev_n_nodes, int *dev_node, int *dev_start, int *dev_feat,
                hipStream_t st);

// The store routes of the tracker (reloc.hip): reloc_run with the candidates read from a store, optionally chosen by
// the database.  reloc_store_prepare sizes the route's own buffers (first call) before anything is enqueued.
struct RelocStoreArgs {
  const vo_kfstore *store;
  const vo_vocab *vocab;
  const int *dev_n_cand, *dev_cand;  // device [B], [B][cand_stride]; ignored with a database
  int cand_stride;
  vo_kfdb *db;                       // or NULL
  const float *dev_stale;
  hipEvent_t *tev;                   // 8 events (featvec, gather, local ids, walk: begin / end) or NULL
};
// `walk`, `err`: the tracker's BoW walk buffers (reserved by the caller) and its sticky word of the store routes (bit 0:
// more candidates than the route holds, bit 1: a key-frame number outside the store), shared with trackRefKeyFrame's
// store route (tracker.hip)
int reloc_store_prepare(Reloc *r, BowWalkBufs *walk, int *err, bool with_db, hipStream_t st);
int reloc_run_store(Reloc *r, const RelocShared &S, const RelocStoreArgs &A);
// (bits 2, 3: vo_tracker_build_local_map -- more distinct local points than max_local, more voters than the list holds)
enum { kStoreErrTooMany = 1, kStoreErrBadId = 2, kStoreErrLocalPoints = 4, kStoreErrLocalKfs = 8 };
bool reloc_last_was_store(const Reloc *r);
// the frames' slot ids in the store's id space [B][cap] and the winners [B] a store route left (VO_ERR_INVALID otherwise)
int reloc_frame_ids(Reloc *r, int **fid, const int **winner);

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

// vo_set_option's process-wide values as last set, 0 before (vo_common.hip): VO_OPT_BA_GRAPH (ba.hip), VO_OPT_POSE_BLOCK
// (pose_only.hip), VO_OPT_BA_PAIRS_KERNEL (ba.hip), VO_OPT_HAMMING_KERNEL (match.hip: 0 = matrix-core form, 1 = VALU form)
int opt_ba_graph();
int opt_pose_block();
int opt_pairs_kernel();
int opt_hamming_kernel();

// Device addresses of the handles' sticky error flags (NULL before the first use): vo_tracker copies them into its
// result block so that one download answers "pose + counts + did anything overflow" (orb.hip, guided.hip).
const int *orb_error_flag(const vo_orb *h);
const int *guided_error_flag(const vo_frames *h);

}  // namespace vo
