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
// the 16-byte granule the arrays of a laid-out block start on
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

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
// what vo_kfstore_create_keyframe_from_frames reads beyond the view (guided.hip): the depth column [slots][cap], the number of
// slots, and the stream the slots were last written on (vo_frames_build_dev, vo_frames_upload)
struct FrameStoreSource {
  const float *depth;
  int slots;
  hipStream_t producer;
};
FrameStoreSource frame_store_source(const vo_frames *h);

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

// k_sim3 (sim3.hip) on device-resident inputs: problem p owns off[p] .. off[p + 1]; nothing is copied or synchronised
int sim3_solve_dev(int n_problems, int fix_scale, const int *off, const double *Pm, const double *pxc, const double *isc, const double *Pc,
                   const double *pxm, const double *ism, const double *cam4, double *poses, double *scales, uint8_t *outlier, int *n_inliers,
                   vo_lm_summary *sums, hipStream_t st);

// vo_kfdb_query_reloc_dev on a stream of the caller's (kfdb.hip): the database's own stream and `st` are ordered around the
// query by events.  Nothing is validated beyond what vo_kfdb_query_reloc_dev checks.
void kfdb_info(const vo_kfdb *db, int *size, int *max_batch);
int kfdb_query_reloc_on(vo_kfdb *db, hipStream_t st, int n_queries, const int32_t *q_start, const int32_t *q_words,
                        const double *q_values, const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand);
// The loop query of ONE key-frame of the database on a stream of the caller's (the store's: detect_loop.hip), ordered the same
// way.  The query's BoW vector is a row of the database itself: dev_q_start [2] = (kf_start[k], kf_start[k + 1]), or an empty
// pair for "no query".  k_kfdb_min_score writes detectLoop's minScore over dev_conn to dev_min_score [1] (1.0f for an empty
// list), and k_kfdb_query takes it from there.  kfdb_dev_view: the rows a store kernel reads (kf_start) or refreshes (the
// neighbour rows); kfdb_order_before makes `st` wait for what the database's stream holds now.
struct KfdbDevView {
  int size, max_kf;
  const int *kf_start;
  int *nbr_n, *nbr;
};
KfdbDevView kfdb_dev_view(const vo_kfdb *db);
int kfdb_order_before(vo_kfdb *db, hipStream_t st);
int kfdb_query_loop_on(vo_kfdb *db, hipStream_t st, const int32_t *dev_q_start, const int32_t *dev_excl_start, const int32_t *dev_excl,
                       const int32_t *dev_conn_start, const int32_t *dev_conn, float *dev_min_score, int max_out, int32_t *n_cand,
                       int32_t *cand);

// ---- searchByBoW against key-frames of a store with the common-node walk on the device (match.hip): k_bow_transform and
// k_featvec build every resident frame's FeatureVector; k_bow_walk writes every (frame, candidate) pair's query list and
// argument block; k_node_replay runs as in bow_search_resident.  All buffers are sized once from (B, cap, per, NK).  A
// tracker owns ONE set, shared by its store routes: relocalisation walks `per` candidates per frame, trackRefKeyFrame one.
// (bow_walk_replay, which reads a store's view: kfstore.h)
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
// the FeatureVector of n features from their node ids (device arrays): n_nodes into *dev_n_nodes, node [n] ascending,
// start [n + 1], feat [n] (the features of a node in index order); n <= 16384.  dev_n: NULL, or a device count that replaces n
// (clamped to [0, n]: the arrays are sized by n)
int featvec_dev(int n, const int *dev_node_of_feature, int *dev_n_nodes, int *dev_node, int *dev_start, int *dev_feat,
                hipStream_t st, const int *dev_n = nullptr);

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
