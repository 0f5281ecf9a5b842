/*
 * vo_hip.h -- C-ABI of the MI355X (gfx950) implementation of the ORB front end and the
 * bundle-adjustment back end of guisongchen/vo_slam_test.
 *
 * This is the drop-in boundary: the reference has no plugin/FFI interface (its hot path is three
 * C++ classes inside libvo.so), so each entry point below names the reference member it replaces.
 * C++ shims with the reference's class names live in include/myslam_shim/ and call only this
 * header.  Plain pointers and sizes; no C++, torch, OpenCV, Eigen or Ceres types.
 *
 * Conventions
 *   - every function returns VO_OK (0) or a negative vo_status; nothing throws.
 *   - "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory (HBM).
 *   - handles are not re-entrant (like ORBextractor, which mutates mvImagePyramid); use one
 *     handle per host thread.  Each handle owns one HIP stream unless one is supplied.
 *   - the library fails loudly (VO_ERR_NO_DEVICE) when no gfx950 device is usable; there is no
 *     CPU fallback.
 */
#ifndef VO_HIP_H
#define VO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  VO_OK = 0,
  VO_ERR_INVALID = -1,   /* bad argument */
  VO_ERR_NO_DEVICE = -2, /* no usable HIP device */
  VO_ERR_HIP = -3,       /* a HIP runtime call failed (vo_last_error() has the text) */
  VO_ERR_CAPACITY = -4,  /* an internal or caller buffer is too small */
  VO_ERR_STOPPED = -5    /* local BA aborted by the stop flag before the first solve */
} vo_status;

const char *vo_last_error(void);
int vo_device_count(void);
const char *vo_version(void);
/* The stateless entry points (vo_hamming_matrix, vo_match_*, vo_pose_only_solve, vo_sim3_solve, vo_pose_graph_solve,
 * vo_chol_solve, ...) keep grow-only device scratch per calling host thread, so that the hot path neither allocates
 * nor frees (the reference's Matcher / Optimizer are called from three threads).  This
 * frees what the calling thread holds and returns the number of bytes; the buffers grow again on the next call.
 * Call it before a worker thread exits, or after a one-off large problem (a 500-key-frame pose graph holds 150 MB). */
size_t vo_release_thread_scratch(void);

/* cv::KeyPoint memory layout (28 bytes) so that the shim can reinterpret the output array. */
typedef struct {
  float x, y;     /* pt, level-0 pixel coordinates */
  float size;     /* 31 * scale[octave], truncated (ORBextractor.cpp:842) */
  float angle;    /* degrees [0,360) from the intensity centroid */
  float response; /* FAST score */
  int32_t octave;
  int32_t class_id; /* -1 */
} vo_keypoint;

/* ------------------------------------------------------------------------------------------
 * ORB extractor  --  replaces ORB_SLAM2::ORBextractor (include/myslam/ORBextractor.h:45-111,
 * src/ORBextractor.cpp).
 * ------------------------------------------------------------------------------------------ */
typedef struct vo_orb vo_orb;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (ORBextractor.cpp:414-476; constructed once at visualOdometry.cpp:31 with 1000,1.2,8,20,7). */
int vo_orb_create(vo_orb **out, int nfeatures, float scale_factor, int nlevels, int ini_th_fast,
                  int min_th_fast);
void vo_orb_destroy(vo_orb *h);
/* run on a caller-owned hipStream_t instead of the handle's own stream (NULL = default stream) */
int vo_orb_set_stream(vo_orb *h, void *hip_stream);
/* VO_ORB_OPT_FUSED_LEVEL_PASS (default 0): 1 = every pyramid level whose geometry allows it is processed by ONE kernel that
 * stages a tile once and produces the level's FAST cell results, its blurred tiles and the next level's rows from it
 * (csrc/orb_level_pass.inc); 0 = the three separate kernels per level.  The results are bit-identical; on MI355X the fused
 * pass measures 6 % slower than the three kernels (profiles/r05_ab_fused.txt: more vector instructions and three workgroup
 * barriers), which is why it is opt-in. */
/* VO_ORB_OPT_EARLY_LEVEL0 (default 0): 1 = outside the instrumented mode (vo_orb_set_timing) FAST on the cells of level 0 and
 * level 0's blur -- the work that needs the caller's image only -- start on the extractor's side stream next to the resize chain;
 * 0 = FAST on all cells behind the pyramid, the whole blur on the side stream next to it.  Results are identical; measured
 * (tools/ext_schedule_ab.py): 2.482 against 2.499 ms per 1024 frames for the extraction alone, no difference for the tracked
 * step (every kernel involved is bound by instruction issue: there is nothing to overlap), hence opt-in. */
/* VO_ORB_OPT_BLUR_KERNEL (default 0): which kernel blurs the levels (identical planes either way): 0 = k_blur_mfma, both passes
 * of the 7x7 filter as int8 matrix-core products with banded weight matrices (levels of at least 64 x 16 pixels with 16-byte
 * aligned rows; the others fall back by themselves), 1 = k_blur_groups, the dot-product form on the VALU. */
/* VO_ORB_OPT_DESCRIBE_BLUR (default 0): 0 = no blurred pyramid is made: the descriptor kernel (k_describe_win) brings the
 * 45 x 45 raw window of a key-point into LDS once, takes the orientation moments from it, blurs it in place (int8 matrix-core
 * products, the arithmetic of the plane kernels: identical descriptors) and runs the tests on it;
 * vo_orb_get_level(blurred = 1) then makes the planes when it is asked for them.  1 = the blurred planes are made for every
 * level of every frame (VO_ORB_OPT_BLUR_KERNEL picks the kernel) and the descriptor kernel (k_describe) reads its windows from
 * them.  The fused level pass (VO_ORB_OPT_FUSED_LEVEL_PASS) makes its own blurred tiles: with it the planes are always used. */
enum { VO_ORB_OPT_FUSED_LEVEL_PASS = 1, VO_ORB_OPT_EARLY_LEVEL0 = 2, VO_ORB_OPT_BLUR_KERNEL = 3, VO_ORB_OPT_DESCRIBE_BLUR = 4 };
int vo_orb_set_option(vo_orb *h, int option, int value);
/* (tests and tools) the fused pass's plan for one level of a width x height image: out = {takes the fused pass, tile pitch,
 * tile rows, score rows, workgroups per frame, LDS bytes per workgroup, survivor-list entries, 0} */
int vo_orb_debug_level_pass(vo_orb *h, int width, int height, int level, int out[8]);

/* GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors (ORBextractor.h:61-76) */
int vo_orb_levels(const vo_orb *h);
float vo_orb_scale_factor(const vo_orb *h);
int vo_orb_scale_factors(const vo_orb *h, float *scale /*nlevels*/, float *inv_scale /*nlevels or NULL*/);
int vo_orb_features_per_level(const vo_orb *h, int *quota /*nlevels*/);
/* upper bound on key-points per frame (the oct-tree may return a few more than nfeatures) */
int vo_orb_max_keypoints(const vo_orb *h);

/* ORBextractor::operator()(image, mask [ignored], keypoints, descriptors)
 * (ORBextractor.cpp:1051-1112; called from Frame::Frame, frame.cpp:22).
 * Host 8-bit grey image in, host key-points (level-major, oct-tree order) and 32-byte descriptors
 * out.  image == NULL or width/height <= 0 returns VO_OK without touching the outputs (:1054). */
int vo_orb_extract(vo_orb *h, const uint8_t *image, int width, int height, int stride,
                   vo_keypoint *keypoints, uint8_t *descriptors, int capacity, int *n_keypoints);

/* The same operator over a batch of frames that is already resident in HBM (bench / pipelines
 * that keep frames on the device).  Frame f starts at dev_images + f*frame_stride_bytes.
 * Outputs are device arrays: key-points [n_frames][capacity], descriptors [n_frames][capacity][32],
 * counts [n_frames].  Asynchronous on the handle's stream; call vo_orb_sync before reading. */
int vo_orb_extract_batch_dev(vo_orb *h, const uint8_t *dev_images, int n_frames, int width,
                             int height, int stride, size_t frame_stride_bytes,
                             vo_keypoint *dev_keypoints, uint8_t *dev_descriptors, int capacity,
                             int32_t *dev_counts);
int vo_orb_sync(vo_orb *h);

/* mvImagePyramid[level] of frame `frame` of the last call (ORBextractor.h:85), unpadded, to host.
 * blurred != 0 returns the 7x7 Gaussian-blurred plane the descriptors were sampled from. */
int vo_orb_get_level(vo_orb *h, int frame, int level, int blurred, uint8_t *dst, int dst_stride,
                     int *width, int *height);
/* FAST candidates of one level of one frame after the per-cell NMS, in reference order
 * (vToDistributeKeys, ORBextractor.cpp:826-833): x,y relative to the (16,16) border, score. */
int vo_orb_get_candidates(vo_orb *h, int frame, int level, float *x, float *y, float *response,
                          int capacity, int *n);
/* per-level key-point counts of one frame of the last call */
int vo_orb_get_level_counts(vo_orb *h, int frame, int32_t *counts /*nlevels*/);

/* Per-stage timing with HIP events recorded on the handle's stream around each stage of every
 * subsequent call (bench.py's live roofline measurement).  Stages: 0 pyramid (all resize launches),
 * 1 FAST cells, 2 oct-tree, 3 offsets (always 0: folded into the descriptor kernel), 4 blur,
 * 5 orientation+descriptor.  With the fused level pass (vo_orb_set_option) stage 0 carries the whole chain of level passes
 * -- pyramid + FAST + blur -- and stages 1 and 4 are empty.  vo_orb_get_timing
 * synchronises, adds the elapsed times of the calls since the last reset to ms[VO_ORB_STAGES],
 * returns the number of timed calls in *n_calls and resets the accumulators. */
#define VO_ORB_STAGES 6
/* Stage hook: `hook(stage, hip_stream, user)` is called on the calling host thread inside vo_orb_extract* each time the launches
 * of a stage (numbering of vo_orb_get_timing: 0 pyramid, 1 FAST, 2 oct-tree, 4 blur, 5 descriptors) have been enqueued on
 * `hip_stream` -- the place to record an event or to make another stream wait, e.g. to start the all-pairs matching of the
 * PREVIOUS batch (matrix cores + HBM writes) on a second stream exactly when this batch's FAST (vector-issue bound) starts:
 * bench.py's extract + match leg does that.  The hook must not synchronise.  NULL removes it. */
typedef void (*vo_orb_stage_hook)(int stage, void *hip_stream, void *user);
int vo_orb_set_stage_hook(vo_orb *h, vo_orb_stage_hook hook, void *user);
int vo_orb_set_timing(vo_orb *h, int enabled);
int vo_orb_get_timing(vo_orb *h, double *ms /*VO_ORB_STAGES*/, int *n_calls);

/* ------------------------------------------------------------------------------------------
 * Matcher  --  replaces the arithmetic of myslam::Matcher (include/myslam/matcher.h:9-45,
 * src/matcher.cpp).  The pointer-graph gather/scatter stays in the C++ shim.
 * ------------------------------------------------------------------------------------------ */

/* Matcher::computeDistance (matcher.cpp:1240-1256) for all pairs: D[i*nb + j] = Hamming(A_i,B_j).
 * Device pointers; descriptors are 32 bytes each, 4-byte aligned. */
int vo_hamming_matrix_dev(const uint8_t *dev_a, int na, const uint8_t *dev_b, int nb,
                          uint16_t *dev_d, void *hip_stream);
/* batched: pair p uses A + p*a_stride, B + p*b_stride, D + p*d_stride (strides in elements of
 * the respective arrays' rows: descriptors / descriptors / uint16) */
int vo_hamming_matrix_batch_dev(const uint8_t *dev_a, int na, size_t a_stride, const uint8_t *dev_b,
                                int nb, size_t b_stride, uint16_t *dev_d, size_t d_stride,
                                int n_pairs, void *hip_stream);
/* host convenience wrapper (copies in/out) -- also what MapPoint::computeDescriptor's N x N
 * median selection (mappoint.cpp:140-151) consumes */
int vo_hamming_matrix(const uint8_t *a, int na, const uint8_t *b, int nb, uint16_t *d);

/* MapPoint::computeDescriptor (mappoint.cpp:118-179): for each set s (one map point) of
 * descriptors desc[offsets[s] .. offsets[s+1]) -- the rows kf->descriptors_.row(idx) of its good
 * observers -- the index (within the set) of the descriptor with the smallest median Hamming
 * distance to all members (:140-172); -1 for an empty set (:136-137 returns without choosing).
 * ONE kernel launch for the whole batch (the N x N distances never leave the GPU); at most 1024
 * observations per map point.  Host pointers.  (The scalar Matcher::computeDistance of two
 * descriptors is a host inline popcount in the shim: a GPU round trip per pair would be absurd.) */
int vo_median_descriptor(const uint8_t *desc, int n_sets, const int32_t *offsets, int32_t *best_idx);


/* one frame's features as the matcher sees them (Frame members, frame.h:26-45) */
typedef struct vo_frame_view_s {
  int32_t n;
  const float *x, *y;       /* unKeypoints_[i].pt */
  const int32_t *octave;    /* unKeypoints_[i].octave */
  const float *angle;       /* unKeypoints_[i].angle */
  const float *uright;      /* uRight_[i] */
  const uint8_t *desc;      /* descriptors_ (n x 32) */
  float xmin, ymin, xmax, ymax; /* Camera::xMin_.. (camera.cpp:40-43) */
} vo_frame_view;

/* ------------------------------------------------------------------------------------------
 * Device-resident frames  --  Frame::undistortKeyPoints / findDepth / assignFeaturesToGrid
 * (frame.cpp:36-133) and Frame/KeyFrame::getFeaturesInArea (frame.cpp:199-247,
 * keyframe.cpp:268-312) on the GPU: key-points stay in HBM between the extractor and the matcher.
 * A vo_frames handle stores up to max_frames frames of up to max_features (<= 16384) features:
 * undistorted key-points, octave, angle, uRight, depth, descriptors and the 64 x 48 grid as CSR.
 * ------------------------------------------------------------------------------------------ */
typedef struct vo_frames vo_frames;
int vo_frames_create(vo_frames **out, int max_frames, int max_features);
void vo_frames_destroy(vo_frames *h);
int vo_frames_capacity(const vo_frames *h, int *max_frames, int *max_features);
/* Camera (camera.cpp:8-47): intrinsics = fx, fy, cx, cy, bf; dist_coef = k1, k2, p1, p2, k3 (NULL or
 * k1 == 0: no undistortion, frame.cpp:41-45); image bounds xMin = yMin = 0, xMax = width, yMax = height. */
int vo_frames_set_camera(vo_frames *h, const float intrinsics[5], const float dist_coef[5], float width,
                         float height);
/* Frame::Frame post-processing (frame.cpp:27-32) of n_frames extractor outputs into slots
 * slot0 ..: dev_keypoints [n_frames][capacity], dev_descriptors [n_frames][capacity][32], dev_counts
 * [n_frames] exactly as vo_orb_extract_batch_dev wrote them.  depth_kind 0: no depth (uRight = depth
 * = -1); 1: float32 metres [h][depth_pitch_bytes]; 2: uint16 raw, metres = raw * inv_depth_scale
 * (Mat::convertTo, visualOdometry.cpp:162-163).  cv::undistortPoints = OpenCV 3.x: 5 fixed-point
 * iterations in double.  Asynchronous on hip_stream. */
int vo_frames_build_dev(vo_frames *h, int slot0, int n_frames, const vo_keypoint *dev_keypoints,
                        const uint8_t *dev_descriptors, const int32_t *dev_counts, int capacity,
                        const void *dev_depth, int depth_kind, size_t depth_frame_stride_bytes,
                        int depth_pitch_bytes, float inv_depth_scale, void *hip_stream);
/* Frame::Frame (frame.cpp:14-34) for one host image in one call: ORB extraction (:22), undistortKeyPoints,
 * findDepth, assignFeaturesToGrid (:27-31) on the device -- the image goes up once, nothing comes back but
 * the raw key-points (Frame::keypoints_, written here) and what vo_frames_download then returns for the slot
 * (unKeypoints_, uRight_, depth_, descriptors_, the grid).  The extractor handle is switched to the calling
 * thread's stream.  depth as in vo_frames_build_dev (host pointer). */
int vo_frames_construct(vo_frames *h, int slot, vo_orb *orb, const uint8_t *image, int width, int height, int stride,
                        const void *depth, int depth_kind, int depth_pitch_bytes, float inv_depth_scale,
                        vo_keypoint *keypoints, int capacity, int *n_keypoints);
/* one already post-processed frame from host arrays (builds the grid); depth may be NULL */
int vo_frames_upload(vo_frames *h, int slot, const vo_frame_view *view, const float *depth,
                     void *hip_stream);
/* copy a slot back (tests / shims): any output may be NULL; cell_start has 64*48+1 entries
 * (cell = ix * 48 + iy), cell_items n entries (feature indices in push_back order). */
int vo_frames_download(vo_frames *h, int slot, int *n, float *x, float *y, int32_t *octave, float *angle,
                       float *uright, float *depth, uint8_t *desc, int32_t *cell_start,
                       uint16_t *cell_items, void *hip_stream);

/* Frame::getFeaturesInArea(u, v, radius, minLevel, maxLevel) (frame.cpp:199-247) and
 * KeyFrame::getFeaturesInArea(u, v, radius) (keyframe.cpp:268-312; min_level = max_level = NULL) for
 * n_queries windows of one stored frame: out_idx[q * max_out + k] = k-th feature index of window q in
 * the reference's order (grid column by column, cells top to bottom, insertion order inside a cell),
 * out_count[q] = number of features in the window (may exceed max_out: the list is then truncated).
 * Host arrays in and out; runs on the calling thread's stream.  The searches above do not go through
 * this list -- they walk the same windows inside their candidate kernel -- it is the reference's
 * accessor for other callers and the direct test of the grid. */
int vo_frames_features_in_area(vo_frames *h, int slot, int n_queries, const float *u, const float *v,
                               const float *radius, const int32_t *min_level, const int32_t *max_level,
                               int32_t *out_idx, int max_out, int32_t *out_count);

/* Guided (window) matching on device-resident frames, batched over frames: frame f of the call
 * searches slot slot0 + f with its own block of queries (query q of frame f at index
 * f * stride + q of every array; all device pointers).
 *   mode 0  searchByProjection(Frame*, Frame*)     matcher.cpp:18-148   aux = 1/z, level = last octave
 *   mode 1  searchByProjection(Frame*, MapPoints)  :274-353             aux = trackProj_uR_, viewcos
 *   mode 2  searchByProjection(Frame*, KeyFrame*)  :150-272             radius, dist_threshold
 *   mode 3  fuseMapPoints candidate search         :1064-1106           aux = projected uR; radius = threshold
 *   mode 4  searchBySim3 / fuseByPose inner search :756-786, :1196-1213 max_dist
 *   mode 5  searchByProjection(KeyFrame*, Sim3&)   :356-447 (Q-M1)      radius = th
 * Modes 0, 1, 2, 5 claim features: dev_assigned [n_frames][max_features] in/out (query index per
 * feature or -1; mode 5 starts from -1), dev_feature_mask [n_frames][max_features] or NULL =
 * blocked / holds-a-map-point / occupied on entry.  Modes 3, 4: dev_best_idx [n_frames][stride].
 * dev_n_matches [n_frames].  Every query owns 32 candidate records; pool_per_frame sizes the per-frame
 * overflow area that windows with more gated candidates spill into (0 = 16 per query);
 * vo_match_guided_status reports an exhausted overflow area after the stream has been synchronised. */
typedef struct {
  int32_t n_queries;          /* queries per frame (upper bound when n_per_frame is given) */
  int32_t stride;             /* distance between the query blocks of consecutive frames (>= n_queries) */
  const int32_t *n_per_frame; /* device, or NULL; a NEGATIVE entry leaves the frame out of the call: nothing of it is
                                 read or written (assigned, best_idx, n_matches keep their values) */
  const uint8_t *flags;       /* bit 0 valid, bit 1 the query's map point has observations (see below) */
  const float *u, *v, *aux;
  const int32_t *level;
  const float *angle, *viewcos; /* modes 0, 2 (checkRot) / mode 1 */
  const uint8_t *desc;
} vo_guided_queries;
typedef struct {
  int32_t mode;
  float radius, bf, ratio, dist_threshold;
  int32_t direction, check_rot, n_levels, max_dist;
  const float *scale_factors; /* host, n_levels entries */
  /* mode 0 only, or NULL: trackWithMotion's retry (visualOdometry.cpp:241-245) decided on the device.  A frame that ends
   * the call with fewer than retry_below matches has its dev_assigned entries set back to -1 and
   * retry_n_per_frame[f] = its query count; every other frame gets -1 -- the n_per_frame array of a second call
   * (same queries, wider radius) that then looks at those frames only. */
  int32_t retry_below;
  int32_t *retry_n_per_frame; /* device [n_frames] */
} vo_guided_params;
int vo_match_guided_dev(vo_frames *h, int slot0, int n_frames, const vo_guided_queries *q,
                        const vo_guided_params *p, const uint8_t *dev_feature_mask, int32_t *dev_assigned,
                        int32_t *dev_best_idx, int32_t *dev_n_matches, size_t pool_per_frame,
                        void *hip_stream);
int vo_match_guided_status(vo_frames *h, void *hip_stream);

/* q_flags bit 0: query valid (map point exists, not outlier, projects inside the image);
 *         bit 1: its map point has observe_cnt_ > 0 (claims the feature for later queries). */

/* Matcher::searchByProjection(Frame* cur, Frame* last, radius, checkRot) (matcher.cpp:18-148).
 * direction: 1 = forward, 2 = backward, 0 = neither (:47-48,:70-75).  assigned[cur.n] in/out:
 * query index matched to each feature or -1.  blocked[cur.n]: feature already holds an observed
 * map point.  Host-array form of vo_match_guided_dev mode 0: the frame view and the queries are
 * uploaded in one block, window search, gates, Hamming distances and the ordered claim replay run on
 * the device, only assigned[] comes back.  Returns the match count in *n_matches. */
int vo_match_frame_projection(const vo_frame_view *cur, int nq, const uint8_t *q_flags,
                              const float *q_u, const float *q_v, const float *q_invz,
                              const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                              float radius, float bf, int direction, int check_rot, int n_levels,
                              const float *scale_factors, const uint8_t *blocked,
                              int32_t *assigned, int *n_matches);

/* Matcher::searchByProjection(Frame*, const vector<MapPoint*>&, thRadius) (matcher.cpp:274-353);
 * ratio = Matcher::ratio_. */
int vo_match_local_map(const vo_frame_view *cur, int nq, const uint8_t *q_flags, const float *q_u,
                       const float *q_v, const float *q_ur, const int32_t *q_level,
                       const float *q_viewcos, const uint8_t *q_desc, float th_radius, float ratio,
                       const float *scale_factors, const uint8_t *blocked, int32_t *assigned,
                       int *n_matches);

/* Matcher::searchByProjection(Frame*, KeyFrame*, radius, distThreshold, found, checkRot)
 * (matcher.cpp:150-272, relocalisation top-up).  Query i = key-frame map point i, already projected
 * (flag bit 0: exists, not bad, not in `found`, z > 0, inside the image and its distance range);
 * q_level = MapPoint::predictScale.  has_map_point[cur.n]: the feature holds any map point (:218);
 * features assigned earlier in the call are skipped as well. */
int vo_match_frame_keyframe(const vo_frame_view *cur, int nq, const uint8_t *q_flags, const float *q_u,
                            const float *q_v, const int32_t *q_level, const float *q_angle,
                            const uint8_t *q_desc, float radius, float dist_threshold, int check_rot,
                            const float *scale_factors, const uint8_t *has_map_point, int32_t *assigned,
                            int *n_matches);

/* DBoW3::FeatureVector of one frame as CSR: node ids ascending, node k owns
 * feat[start[k] .. start[k+1]) (frame.h:50, keyframe.h). */
typedef struct {
  int32_t n_nodes;
  const uint32_t *node_id;
  const int32_t *start;
  const uint32_t *feat;
} vo_bow_view;

/* Matcher::searchByBoW(KeyFrame*, Frame*, matches, checkRot) (matcher.cpp:449-559; mode 0:
 * match[b.n] = A index held by each B feature) and searchByBoW(KeyFrame*, KeyFrame*, ...)
 * (:561-677; mode 1: match[a.n] = B index of each A feature).  a_valid / b_valid: the feature has
 * a good map point.  ratio = Matcher::ratio_.  Runs on the device (k_node_replay: the node-by-node
 * claims in the reference's order, distances computed on the fly); b.n <= 16384, else VO_ERR_CAPACITY. */
int vo_match_bow(const vo_frame_view *a, const uint8_t *a_valid, const vo_bow_view *a_nodes,
                 const vo_frame_view *b, const uint8_t *b_valid, const vo_bow_view *b_nodes, int mode,
                 float ratio, int check_rot, int32_t *match, int *n_matches);

/* The same search for n_pairs pairs in ONE launch (one workgroup per pair; frames that appear in several pairs are
 * uploaded once): the searchByBoW calls over the relocalisation candidates (visualOdometry.cpp:354-371) or the loop
 * candidates (loopClosing.cpp:182).  Arrays of n_pairs pointers; match[p] has b[p]->n (mode 0) or a[p]->n (mode 1)
 * entries; results identical to n_pairs single calls. */
int vo_match_bow_batch(int n_pairs, const vo_frame_view *const *a, const uint8_t *const *a_valid,
                       const vo_bow_view *const *a_nodes, const vo_frame_view *const *b, const uint8_t *const *b_valid,
                       const vo_bow_view *const *b_nodes, int mode, float ratio, int check_rot, int32_t *const *match,
                       int *n_matches);

/* Matcher::searchForTriangulation(kf1, kf2, matchIdxs, F12, checkRot) (matcher.cpp:867-1010,
 * called at localMapping.cpp:187).  *_has_map_point: feature already triangulated (skipped).
 * F12 row-major; (ex, ey) = camera centre 1 projected into key-frame 2 (:887-891).
 * match12[a.n] = B index or -1.  Same device kernel as vo_match_bow (epipole / epipolar-line gates per
 * candidate); scale_factors: 8 entries. */
int vo_match_triangulation(const vo_frame_view *a, const uint8_t *a_has_map_point, const vo_bow_view *a_nodes,
                           const vo_frame_view *b, const uint8_t *b_has_map_point, const vo_bow_view *b_nodes,
                           const double F12[9], float ex, float ey, const float *scale_factors,
                           int check_rot, int32_t *match12, int *n_matches);

/* matching part of Matcher::fuseMapPoints (matcher.cpp:1012-1133; the map mutation :1108-1127
 * stays in the shim).  Query = candidate map point projected into the key-frame (flag bit 0:
 * passes the gates of :1029-1062); best_idx[nq] = feature to fuse with or -1. */
int vo_match_fuse(const vo_frame_view *kf, int nq, const uint8_t *q_flags, const float *q_u,
                  const float *q_v, const float *q_ur, const int32_t *q_level, const uint8_t *q_desc,
                  float threshold, const float *scale_factors, int32_t *best_idx, int *n_matches);

/* Bag-of-words transform: DBoW3::Vocabulary::transform(features, bowVec, featVec, levelsup) as called by
 * Frame::computeBow (frame.cpp:248-253) and KeyFrame::computeBow (keyframe.cpp:394-398), levelsup = 3.
 * The vocabulary tree (parsed on the host from the DBoW3 file) is uploaded once as flat arrays: the
 * children of node i are children[child_start[i] .. child_start[i+1]), node 0 is the root,
 * word_id[i] >= 0 marks a leaf (a word) with weight node_weight[i], node_desc holds one 32-byte ORB
 * descriptor per node.  Per feature: the word, its weight, and the node reached at level
 * depth_L - levelsup (the key of the FeatureVector that searchByBoW / searchForTriangulation walk).
 * The (word -> summed weight) map and its L1 normalisation are vo_bow_vector below (or std::map insertions
 * in the shim); the (node -> feature list) map stays in the shim. */
typedef struct vo_vocab vo_vocab;
int vo_vocab_create(vo_vocab **out, int n_nodes, int depth_L, const int32_t *child_start, const int32_t *children,
                    const uint8_t *node_desc, const double *node_weight, const int32_t *word_id);
void vo_vocab_destroy(vo_vocab *v);
int vo_bow_transform(const vo_vocab *v, int n, const uint8_t *desc, int levelsup, int32_t *word_id, double *weight,
                     int32_t *node_id);

/* The vocabulary file itself (DBoW3::Vocabulary(path), vo_run.cpp:87): DBoW3's binary stream
 * (Vocabulary::toStream; plain, or -- what Vocabulary::save(path) writes by default, reference map.cpp:94 -- in QuickLZ
 * level-1 chunks, decoded by a restatement of the published decoder: no library-written file was available to pin it,
 * a stream that does not follow the format is refused), its cv::FileStorage form (.yml / .yml.gz: Vocabulary::save(cv::FileStorage&),
 * what DBoW3::Vocabulary(path) falls back to) or the ORB-SLAM2 text format; builds the device tree. */
int vo_vocab_load(const char *path, vo_vocab **out, int *n_nodes, int *n_words, int *branching_k, int *depth_L);
/* Map::createVocabulary (map.cpp:60-99): DBoW3::Vocabulary::create(descriptors) with k children per node and L levels,
 * TF-IDF weights -- the k-majority tree (k-means++ seeding, Lloyd with per-bit majority centres, idf of the training
 * set's own transform), trained on the device.  DBoW3 is unpinned and seeds itself from the clock: the contract (integer
 * draw keyed by (seed, the node's path), breadth-first node ids, every deviation) is DESIGN.md section 4d; a tree is a
 * function of (descriptors in order, image_offsets, k, L, seed) alone.  desc: n_desc x 32 bytes in the order
 * createVocabulary concatenates them; image_offsets[n_images + 1]: CSR of the images (key-frames / lost frames) over the
 * descriptors, starting at 0, ascending, ending at n_desc.  k < 2, L < 1, n_desc < 0 or bad offsets: VO_ERR_INVALID;
 * k > VO_VOCAB_MAX_K, L > VO_VOCAB_MAX_L or n_desc > VO_VOCAB_MAX_DESC: VO_ERR_CAPACITY; *out is written on success
 * only.  n_desc == 0 gives a root-only tree.  A clustering that still moves after VO_VOCAB_MAX_LLOYD assignments keeps its
 * last one and is counted in info->n_capped.  The _dev form takes device arrays (descriptors 4-byte aligned) and works on
 * hip_stream (NULL: the legacy stream); both forms synchronise (one word per Lloyd iteration, the tree's bookkeeping once
 * per level) and allocate their own buffers: a one-off at the end of a run, like the reference's. */
#define VO_VOCAB_MAX_K 32
#define VO_VOCAB_MAX_L 16
#define VO_VOCAB_MAX_DESC (1 << 23)
#define VO_VOCAB_MAX_LLOYD 2048
typedef struct { int32_t n_nodes, n_words, n_levels, lloyd_iterations_max, n_capped; } vo_vocab_train_info;
int vo_vocab_train(int n_desc, const uint8_t *desc, int n_images, const int32_t *image_offsets, int k, int L, uint64_t seed,
                   vo_vocab **out, vo_vocab_train_info *info);
int vo_vocab_train_dev(int n_desc, const uint8_t *dev_desc, int n_images, const int32_t *dev_image_offsets, int k, int L,
                       uint64_t seed, void *hip_stream, vo_vocab **out, vo_vocab_train_info *info);
/* The tree of a handle back on the host, in vo_vocab_create's layout (what map.cpp:60-99 goes on to save).  Any array may
 * be NULL (sizes only); children needs child_start[n_nodes] entries, which is n_nodes - 1 for a tree. */
int vo_vocab_tree(const vo_vocab *v, int *n_nodes, int *depth_L, int32_t *child_start, int32_t *children, uint8_t *node_desc,
                  double *node_weight, int32_t *word_id);
/* vocab.save(path) of map.cpp:60-99: DBoW3's Vocabulary::toStream, uncompressed (the plain binary stream vo_vocab_load
 * reads; DBoW3 reads it too, its QuickLZ form is not written).  k is recorded in the file's header (2 .. 64). */
int vo_vocab_save(const vo_vocab *v, int k, const char *path);

/* Map::score (map.cpp:335-376): L1 similarity of the query BoW vector (ascending word ids) with every
 * candidate's (CSR: candidate c owns cand_words / cand_values [cand_start[c], cand_start[c+1])); one
 * launch for all candidates of detectLoopCandidates / detectRelocalizationCandidates (:210-333). */
int vo_bow_score(int n_query, const int32_t *query_words, const double *query_values, int n_candidates,
                 const int32_t *cand_start, const int32_t *cand_words, const double *cand_values, double *scores);

/* The BoW vector of DBoW3::Vocabulary::transform for a ragged batch of frames: frame f owns the per-feature (word, weight)
 * pairs feat_start[f] .. feat_start[f+1] as vo_bow_transform writes them.  Features with weight <= 0 are skipped, the
 * weights of one word are added in FP64 in feature order, the L1 norm is the FP64 sum of fabs(value) in ascending word
 * order and every value is divided by it when it is > 0: bitwise what BowVector::addWeight / normalize(L1) give.  Output
 * as CSR: out_start[n_frames + 1], ascending distinct words and their values (room for as many entries as features).
 * The _dev form takes device arrays and enqueues three launches on hip_stream.  Its intermediate result lives in scratch of
 * the calling host thread that only grows: a call that needs more than any earlier call of the thread reallocates it
 * (hipFree: a device synchronisation, once per size), every other call synchronises nothing.  Because the scratch is per
 * thread and not per stream, one host thread must keep its calls on ONE stream (or drain the previous stream first): a second
 * call on another stream would overwrite what the first call's kernels still read. */
int vo_bow_vector(int n_frames, const int32_t *feat_start, const int32_t *word, const double *weight, int32_t *out_start,
                  int32_t *out_words, double *out_values);
int vo_bow_vector_dev(int n_frames, int n_features, const int32_t *dev_feat_start, const int32_t *dev_word, const double *dev_weight,
                      int32_t *dev_out_start, int32_t *dev_out_words, double *dev_out_values, void *hip_stream);

/* The key-frame database: Map::insertKeyFrame's inverted index (map.cpp:9-22),
 * Map::detectRelocalizationCandidates (:101-208) and Map::detectLoopCandidates (:210-333) with the minScore loop of
 * LoopClosing::detectLoop (loopClosing.cpp:71-83), resident on the device and answered for a batch of queries at once.
 * A key-frame is known by its insertion number 0, 1, 2 ...; there is no erase (Map::eraseKeyFrame edits a copy of the
 * posting list and removes nothing) and isBad() is never consulted.  The handle owns every device buffer: all of them are
 * sized at creation from (n_words, max_keyframes, max_words_per_keyframe, max_batch), only the staging of the host forms
 * grows with their arguments.  Exceeding max_keyframes, max_words_per_keyframe, max_batch or max_out is VO_ERR_CAPACITY.
 * Calls on one handle are serialised by the caller (the reference holds mutexMap_); different handles are independent.
 * Work is enqueued on the handle's stream (NULL, the legacy stream, until vo_kfdb_set_stream).
 *
 * insert: the key-frame's BoW vector (vo_bow_vector's output: word ids strictly ascending, checked by the host form).
 * set_neighbors: KeyFrame::getBestCovisibleKFs(10) of an inserted key-frame, in its order (n <= 10, ids already inserted).
 *
 * Queries: query i owns q_words / q_values [q_start[i], q_start[i+1]) (a BoW vector).  n_cand[i] is the true number of
 * candidates, cand [n_queries][max_out] holds the first min(n_cand[i], max_out) of them in the reference's order; the host
 * forms return VO_ERR_CAPACITY when a query has more than max_out (n_cand is still written), the _dev forms leave that
 * comparison to the caller.  score_out [n_queries][size] (or NULL): relocalisation -- the value relocateScore_ holds after
 * query i alone: its Map::score as float where the key-frame was scored, stale_score (NULL = 0.0f) elsewhere; loop -- the
 * loopScore_ written by query i, -1.0f where the key-frame was not scored.  stale_score [size]: relocateScore_ as earlier
 * queries left it, which the reference adds for a neighbour that shares a word but was not scored; results are a pure
 * function of (database, query, stale_score) and do not depend on the batch.
 * Loop query: excl = getConnectKFs() and the key-frame itself (CSR over queries); min_score [n_queries], or NULL: computed
 * as detectLoop does, the float minimum (from 1.0f) of Map::score against conn = the non-bad orderedConnectKFs_ (CSR).
 * The _dev forms take device arrays, allocate nothing and do not synchronise: one launch, preceded by the four launches
 * that rebuild the index when key-frames were inserted since the previous query.  They cannot validate what they do not
 * read: the caller guarantees word ids within [0, n_words), excl / conn ids within [0, size) and at most max_keyframes conn
 * entries per query (the kernels skip anything else, so memory stays safe, but the skip is not reported), and
 * vo_kfdb_insert_dev trusts its words to ascend strictly within [0, n_words) (scores of a key-frame that breaks this are
 * undefined).  The host forms check all of it and return VO_ERR_INVALID. */
typedef struct vo_kfdb vo_kfdb;
int vo_kfdb_create(vo_kfdb **out, int n_words, int max_keyframes, int max_words_per_keyframe, int max_batch);
void vo_kfdb_destroy(vo_kfdb *db);
int vo_kfdb_set_stream(vo_kfdb *db, void *hip_stream);
int vo_kfdb_size(const vo_kfdb *db);
/* VO_KFDB_OPT_LDS_KEYFRAMES: the largest database whose per-query counters are kept in LDS (default and maximum 16384);
 * larger ones use a slab in device memory, with the same results. */
#define VO_KFDB_OPT_LDS_KEYFRAMES 1
int vo_kfdb_set_option(vo_kfdb *db, int option, int value);
int vo_kfdb_insert(vo_kfdb *db, int n, const int32_t *words, const double *values, int32_t *index);
int vo_kfdb_insert_dev(vo_kfdb *db, int n, const int32_t *dev_words, const double *dev_values, int32_t *index);
int vo_kfdb_set_neighbors(vo_kfdb *db, int keyframe, int n, const int32_t *ids);
/* set_neighbors for the key-frames first .. first + count - 1 in one call (two copies, no launch per key-frame):
 * n[count] list lengths (<= 10), ids [count][10] (entries beyond n[k] are ignored). */
int vo_kfdb_set_neighbors_batch(vo_kfdb *db, int first, int count, const int32_t *n, const int32_t *ids);
/* The neighbour row of one key-frame as the database holds it (set_neighbors, or vo_kfstore_detect_loop's refresh): *n its
 * length, ids [10] with -1 beyond it.  Synchronises. */
int vo_kfdb_get_neighbors(vo_kfdb *db, int keyframe, int32_t *n, int32_t *ids /*[10]*/);
int vo_kfdb_query_reloc(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                        const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand, float *score_out);
int vo_kfdb_query_reloc_dev(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                            const float *stale_score, int max_out, int32_t *n_cand, int32_t *cand, float *score_out);
int vo_kfdb_query_loop(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                       const int32_t *excl_start, const int32_t *excl, const float *min_score, const int32_t *conn_start,
                       const int32_t *conn, int max_out, int32_t *n_cand, int32_t *cand, float *score_out);
int vo_kfdb_query_loop_dev(vo_kfdb *db, int n_queries, const int32_t *q_start, const int32_t *q_words, const double *q_values,
                           const int32_t *excl_start, const int32_t *excl, const float *min_score, const int32_t *conn_start,
                           const int32_t *conn, int max_out, int32_t *n_cand, int32_t *cand, float *score_out);

/* cv::solvePnPRansac(pts3d, pts2d, K, noArray(), rvec, tvec, false, iterations, reproj_error, confidence, inliers,
 * SOLVEPNP_EPNP) as VisualOdometry::poseEstimateByPnP calls it (visualOdometry.cpp:778-830: 100, 8.0, 0.99), for a ragged
 * batch: problem p owns correspondences offsets[p] .. offsets[p+1] of pts3d [.][3] (MapPoint::getPose() as float) and
 * pts2d [.][2] (unKeypoints_ pixels); cam4 = fx, fy, cx, cy (the float K), no distortion.  Contract:
 * cv::RNG((uint64)-1) per problem + getSubset 5-tuples, EPnP in FP64 per tuple, float reprojection gate
 * err <= (float)(reproj_error^2), the ordered RANSAC loop with RANSACUpdateNumIters, then EPnP refitted on the winner's
 * inliers (the mask is not recomputed after the refit).  n == 5: one EPnP on all five, all inliers.  n < 5: failure
 * (deviation: the reference runs P3P at n == 4 and throws below).
 * Outputs per problem: Tcw12 [12] (R | t, 3 x 4 row-major; zero on failure), pose6 [6] = se3 log of it (host form only,
 * may be NULL), n_inliers, status (1 found, 0 not); inlier [offsets[P]] the mask.  diag (NULL, or any member NULL):
 * samples [P][iterations][5], counts [P][iterations], hyp_Tcw12 [P][iterations][12] of every hypothesis (including those
 * past the final niters; zero for n <= 5), best_iter [P] (-1: none / n == 5), final_niters [P].
 * Limits: P <= VO_PNP_MAX_PROBLEMS, iterations <= VO_PNP_MAX_ITERATIONS, P x iterations <= VO_PNP_MAX_HYPOTHESES, and (host
 * form, checked) n <= VO_PNP_MAX_POINTS per problem; beyond them VO_ERR_CAPACITY, nothing truncated.
 * The _dev form takes device arrays (diag members too) and enqueues on hip_stream (NULL: the legacy stream) without host
 * synchronisation or allocation; its intermediates live in the caller's device `workspace` of at least
 * vo_pnp_workspace_bytes(n_problems, iterations) bytes (else VO_ERR_CAPACITY), which must not be in use by another call
 * until this one has completed on hip_stream -- calls on different streams take different workspaces.  Its offsets are
 * not inspected on the host (the kernels stage a problem's correspondences in chunks and take any size).  The host form
 * is synchronous and keeps its own buffers.
 * Every output of a problem (and its diag entries) is the same bit for bit whatever its position in the batch and
 * whatever other problems share the call.
 * Degenerate sets: CC^-1 of the barycentric coordinates is the pseudo-inverse cvInvert(CV_SVD) forms (coplanar or
 * coincident points give finite coordinates); a refit whose pose is not finite fails the problem (status 0, no
 * inliers) -- a deviation: OpenCV would return its non-finite pose. */
enum { VO_PNP_MAX_PROBLEMS = 65536, VO_PNP_MAX_ITERATIONS = 1000, VO_PNP_MAX_HYPOTHESES = 1 << 21, VO_PNP_MAX_POINTS = 1 << 20 };
typedef struct {
  int32_t *samples, *counts;
  double *hyp_Tcw12;
  int32_t *best_iter, *final_niters;
} vo_pnp_diag;
int vo_pnp_ransac(int n_problems, const int32_t *offsets, const float *pts3d, const float *pts2d, const float cam4[4],
                  int iterations, float reproj_error, double confidence, double *Tcw12, double *pose6, uint8_t *inlier,
                  int32_t *n_inliers, int32_t *status, const vo_pnp_diag *diag);
size_t vo_pnp_workspace_bytes(int n_problems, int iterations); /* 0 for invalid arguments */
int vo_pnp_ransac_dev(int n_problems, const int32_t *offsets, const float *pts3d, const float *pts2d, const float cam4[4],
                      int iterations, float reproj_error, double confidence, double *Tcw12, uint8_t *inlier, int32_t *n_inliers,
                      int32_t *status, const vo_pnp_diag *diag, void *workspace, size_t workspace_bytes, void *hip_stream);

/* Sim3Solver (src/sim3Solver.cpp): every RANSAC hypothesis of Sim3Solver::iterate in one launch -- Horn's
 * closed form (computeSim3 :179-252) for the three sampled correspondences triplets[3k..3k+2] and
 * checkInliers (:254-280) over all n correspondences.  The random triplets come from the caller (the
 * reference draws them with rand(), :119-137), as does the sequential pick "first hypothesis whose
 * inlier count beats the threshold" (:141-160).  max_err = the reference's INTEGER thresholds
 * (vector<int>, 9.210 sigma^2 truncated).  Per hypothesis: counts[k], inlier_flags[k * n ..] (or NULL),
 * sims[13 k ..] = R12 row-major (9), t12 (3), s12.
 * All six correspondence arrays NULL: the correspondences the calling host thread passed with its previous call (same n)
 * are still on the device and are used again -- a caller that evaluates one hypothesis per call (to keep its random
 * generator in step with the reference's) uploads them once per Sim3Solver::iterate, not once per trip. */
int vo_sim3_ransac_eval(int n, const double *cam1_points, const double *cam2_points, const double *pixels1,
                        const double *pixels2, const int32_t *max_err1, const int32_t *max_err2,
                        const float cam4[4], int n_hypotheses, const int32_t *triplets, int fix_scale,
                        int32_t *counts, uint8_t *inlier_flags, double *sims);

/* LocalMapping::createNewMapPoints' linear triangulation (localMapping.cpp:234-251), batched: normalised
 * observations xn1 / xn2 [n][2], Tcw1 (3 x 4 float, row-major) of the current key-frame, Tcw2 one pose or
 * one per pair.  points [n][3]; ok[i] = 0 where |x_3| < 1e-8 (:245-246 skips the pair).  The right
 * singular vector is taken from the eigen-decomposition of A^T A in double: agreement with cv::SVD's
 * float Jacobi is to float rounding (stated tolerance 1e-4 relative), not bit-exact. */
int vo_triangulate(int n, const float *xn1, const float *xn2, const float Tcw1[12], const float *Tcw2,
                   int per_pair_pose2, float *points, uint8_t *ok);

/* searchForTriangulation of the current key-frame `a` against ALL its neighbours in one launch (the loop of
 * LocalMapping::createNewMapPoints, localMapping.cpp:160-190: <= 10 neighbours, one call each in the reference): pair p
 * searches b[p] with F12 = F[9p .. 9p+8] and the epipole (ex[p], ey[p]); match12[p] has a->n entries.  The calls are
 * independent in the reference (matchIdxs is local to a neighbour), so the results equal n_pairs single calls. */
int vo_match_triangulation_batch(int n_pairs, const vo_frame_view *a, const uint8_t *a_has_map_point,
                                 const vo_bow_view *a_nodes, const vo_frame_view *const *b,
                                 const uint8_t *const *b_has_map_point, const vo_bow_view *const *b_nodes, const double *F,
                                 const float *ex, const float *ey, const float *scale_factors, int check_rot,
                                 int32_t *const *match12, int *n_matches);

/* cv::cvtColor(CV_RGB2GRAY / CV_BGR2GRAY [/ RGBA / BGRA]) of VisualOdometry::createFrame
 * (visualOdometry.cpp:146-159), OpenCV 3.x fixed point. */
int vo_rgb_to_gray(const uint8_t *src, long long n_pixels, int channels, int first_is_red, uint8_t *dst);
int vo_rgb_to_gray_dev(const uint8_t *dev_src, long long n_pixels, int channels, int first_is_red,
                       uint8_t *dev_dst, void *hip_stream);

/* The reference harness's I/O (test/vo_run.cpp): associate.txt (:24-58), cv::imread of 8-bit colour
 * / 16-bit depth PNGs (:108-109; zlib + PNG filters, non-interlaced), the trajectory files (:154-232,
 * Twc7 = translation + quaternion x y z w per pose, Eigen's default stream format) and the tracking-
 * time report (:138-151). */
typedef struct vo_dataset vo_dataset;
int vo_dataset_open(vo_dataset **out, const char *dataset_dir, int max_frames);
int vo_dataset_size(const vo_dataset *d);
int vo_dataset_entry(const vo_dataset *d, int i, const char **rgb_time, const char **rgb_path,
                     const char **depth_time, const char **depth_path);
void vo_dataset_close(vo_dataset *d);
int vo_png_info(const char *path, int *width, int *height, int *channels, int *bit_depth);
int vo_png_read(const char *path, int as_bgr, void *dst, size_t dst_bytes);
int vo_trajectory_write(const char *path, int n, const char *const *timestamps, const double *Twc7);
int vo_tracking_time_stats(const double *seconds, int n_tracked, double *median, double *mean);

/* Loop-closure searches.  All three project map points into a key-frame and take, per point, the
 * best Hamming match among KeyFrame::getFeaturesInArea(u, v, th * scale[level]) with octave in
 * [level - 1, level]; flag bit 0 of a query = it passed the projection gates of the routine.
 *
 * vo_match_area_best: queries independent -- the inner search of Matcher::searchBySim3
 * (matcher.cpp:756-786, 821-851; max_dist = 100) and of Matcher::fuseByPose (:1196-1213;
 * max_dist = 50; the map mutation :1215-1230 stays in the shim). */
int vo_match_area_best(const vo_frame_view *kf, int nq, const uint8_t *q_flags, const float *q_u,
                       const float *q_v, const int32_t *q_level, const uint8_t *q_desc, float th,
                       const float *scale_factors, int max_dist, int32_t *best_idx, int *n_matches);

/* Matcher::searchByProjection(KeyFrame*, Sim3&, loopMapPoints, matchMapPoints, th)
 * (matcher.cpp:356-447).  occupied[kf.n]: matchMapPoints[k] non-null on entry; assigned[kf.n] =
 * query that claimed the feature, or -1.  The reference's skip test `matchMapPoints[j]` (:422)
 * indexes with the candidate counter, not the feature index; reproduced. */
int vo_match_sim3_projection(const vo_frame_view *kf, int nq, const uint8_t *q_flags, const float *q_u,
                             const float *q_v, const int32_t *q_level, const uint8_t *q_desc, int th,
                             const float *scale_factors, const uint8_t *occupied, int32_t *assigned,
                             int *n_matches);

/* Matcher::searchBySim3 (matcher.cpp:679-865): q1 = map point of feature i of key-frame 1 projected
 * into key-frame 2 (flag 0 also for features without a usable point or already matched, :722-727),
 * q2 the reverse; match12[kf1.n] = feature of key-frame 2, kept only when both directions agree. */
int vo_match_sim3_mutual(const vo_frame_view *kf1, const vo_frame_view *kf2, const uint8_t *q1_flags,
                         const float *q1_u, const float *q1_v, const int32_t *q1_level, const uint8_t *q1_desc,
                         const uint8_t *q2_flags, const float *q2_u, const float *q2_v,
                         const int32_t *q2_level, const uint8_t *q2_desc, float th,
                         const float *scale_factors1, const float *scale_factors2, int32_t *match12,
                         int *n_matches);

/* ------------------------------------------------------------------------------------------
 * Optimizer  --  replaces myslam::Optimizer (include/myslam/optimizer_ceres.h:12-97,
 * src/optimizer_ceres.cpp) including the Ceres solve it delegates to.
 * Poses are se3 tangent vectors [upsilon(3); omega(3)] = Sophus SE3::log(Tcw); cam = fx,fy,cx,cy,bf.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t iterations;  /* LM iterations run (successful or not) */
  int32_t accepted;
  int32_t termination; /* 0 max iterations, 1 function tol., 2 parameter tol., 3 gradient tol., 4 failure */
  int32_t reserved;
  double initial_cost, final_cost, final_radius;
} vo_lm_summary;

/* Optimizer::solvePoseOnlySE3(Frame*) (optimizer_ceres.cpp:157-314) for `n_problems` independent
 * frames in one launch (one workgroup per frame).  Problem p owns observations
 * [offsets[p], offsets[p+1]).  obs = (u, v, uR) with uR < 0 for monocular observations.
 * pose [n_problems][6] in/out, outlier[total obs] out, n_inliers[n_problems] out.
 * summaries: NULL or [n_problems][2] (Huber round, plain round).  Host pointers. */
int vo_pose_only_solve(int n_problems, const int32_t *offsets, const double *points,
                       const double *obs, const double *inv_sigma, const double cam[5],
                       double *poses, uint8_t *outlier, int32_t *n_inliers,
                       vo_lm_summary *summaries);
/* device-resident variant (all pointers device memory, asynchronous on hip_stream) */
int vo_pose_only_solve_dev(int n_problems, const int32_t *dev_offsets, int max_obs,
                           const double *dev_points, const double *dev_obs,
                           const double *dev_inv_sigma, const double *dev_cam5, double *dev_poses,
                           uint8_t *dev_outlier, int32_t *dev_n_inliers,
                           vo_lm_summary *dev_summaries, void *hip_stream);

/* the same with explicit ranges: problem p owns observations [ranges[2p], ranges[2p] + ranges[2p+1])
 * (frames laid out at a fixed stride by vo_track_gather_dev) */
int vo_pose_only_solve_ranges_dev(int n_problems, const int32_t *dev_ranges, const double *dev_points,
                                  const double *dev_obs, const double *dev_inv_sigma, const double *dev_cam5,
                                  double *dev_poses, uint8_t *dev_outlier, int32_t *dev_n_inliers,
                                  vo_lm_summary *dev_summaries, void *hip_stream);

/* Tracking glue on the device (a tracked frame stays in HBM from the extractor to the pose):
 *   vo_track_project_dev  projection prologue of searchByProjection(Frame*, Frame*) (matcher.cpp:41-64):
 *       dev_Tcw [n_frames][12] = rotation row-major + translation of the current pose estimate,
 *       dev_points [n_frames][stride][3] the last frame's map points, dev_point_flags bit 0 = point
 *       exists and is no outlier, bit 1 = observe_cnt_ > 0; writes the mode-0 query arrays
 *       (flags, u, v, 1/z) of vo_match_guided_dev.  xmin .. ymax are the int-truncated image bounds.
 *   vo_track_scatter_dev  frame->mappoints_[k] = the query that claimed feature k: copies its world
 *       point into dev_feature_points [n_frames][max_features][3], sets dev_feature_has (and
 *       dev_feature_observed = flag bit 1, the `blocked` mask of the next search).
 *   vo_track_gather_dev   the gather of solvePoseOnlySE3 (optimizer_ceres.cpp:181-202): features that
 *       hold a map point, in feature order, into points / obs (x, y, uRight) / 1/sigma at
 *       [f * max_features ...) with dev_ranges [n_frames][2] = (start, count) for
 *       vo_pose_only_solve_ranges_dev; dev_index (or NULL) = the feature index of every observation. */
int vo_track_project_dev(int n_frames, int n_queries, int stride, const double *dev_Tcw, const double *dev_points,
                         const uint8_t *dev_point_flags, const float cam4[4], int xmin, int xmax, int ymin,
                         int ymax, uint8_t *dev_q_flags, float *dev_u, float *dev_v, float *dev_invz,
                         void *hip_stream);
int vo_track_scatter_dev(vo_frames *h, int slot0, int n_frames, const int32_t *dev_assigned,
                         const double *dev_query_points, const uint8_t *dev_query_flags, int stride,
                         double *dev_feature_points, uint8_t *dev_feature_has, uint8_t *dev_feature_observed,
                         void *hip_stream);
int vo_track_gather_dev(vo_frames *h, int slot0, int n_frames, const double *dev_feature_points,
                        const uint8_t *dev_feature_has, const float *scale_factors, int n_levels,
                        double *dev_points, double *dev_obs, double *dev_inv_sigma, int32_t *dev_ranges,
                        int32_t *dev_index, void *hip_stream);
/* vo_track_scatter_dev followed by vo_track_gather_dev in one launch (same outputs, bit for bit): what the
 * tracker runs between a search and the pose solve that consumes its matches. */
int vo_track_scatter_gather_dev(vo_frames *h, int slot0, int n_frames, const int32_t *dev_assigned,
                                const double *dev_query_points, const uint8_t *dev_query_flags, int stride,
                                double *dev_feature_points, uint8_t *dev_feature_has,
                                uint8_t *dev_feature_observed, const float *scale_factors, int n_levels,
                                double *dev_points, double *dev_obs, double *dev_inv_sigma,
                                int32_t *dev_ranges, int32_t *dev_index, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * The tracked-frame pipeline as one object  --  VisualOdometry::trackWithMotion + trackLocalMap
 * (visualOdometry.cpp:228-251, 286-300, 745-775, 864-886) for a batch of `batch` independent camera
 * streams resident in HBM: extraction, Frame::Frame post-processing, searchByProjection against the last
 * frame's map points (radius 15), solvePoseOnlySE3, cullingOutliersBeforeLocalMap, Frame::isInFrame +
 * MapPoint::predictScale for the local map points WITH THE REFINED POSE, searchByProjection against
 * them (thRadius 3, ratio 0.8), solvePoseOnlySE3, inlier count.  One call enqueues the whole sequence
 * (27 kernel launches) without host synchronisation; batch = 1 with host images is the single-stream form
 * (Frame construction to pose in one call).
 *
 * Streams: the searches and pose solves run on `stream` (NULL: a high-priority stream of the tracker),
 * the extraction on `extract_stream` (NULL: a stream of the tracker, or `stream` itself when
 * single_stream != 0).  Several trackers that share one extract_stream take turns on the extraction
 * while each other's searches and solves run next to it (two batches in flight: bench.py's regime).
 *
 * The retry of trackWithMotion -- fewer than 20 matches: clear, search again at 2 x radius (:241-245) -- runs on the
 * device for the frames that need it (a per-frame flag, a second candidate / replay pass over the flagged frames only).
 * Status bits VO_TRACK_FEW_MATCHES / VO_TRACK_FEW_INLIERS tell the caller that the reference would have left
 * trackWithMotion (:247, :253); the route it takes then is vo_tracker_track_ref_keyframe below (trackRefKeyFrame,
 * :256-277).  Relocalisation (:313-395), the route of a LOST stream, is vo_tracker_relocalize below: the ordered walk
 * over the caller's candidate key-frames (searchByBoW, EPnP RANSAC, solvePoseOnlySE3, the two guided top-ups, the five
 * gates) runs on the device for the whole batch; Map::detectRelocalizationCandidates and the hand-over to trackLocalMap
 * after a success stay caller code on that call.  vo_tracker_relocalize_db / vo_tracker_relocalize_store further below
 * take the candidates from the device key-frame database (vo_kfdb) and read their features from a device store
 * (vo_kfstore): detectRelocalizationCandidates and the walk in one asynchronous call.  Not covered: the map-side steps between the two stages:
 * trackLocalMap derives localKeyframes_ / localMappoints_ from frame_curr_->mappoints_ AFTER the first stage's culling
 * (updateLocalKeyFrames / updateLocalMapPoints, :286-291), whereas this call takes the local map BEFORE it starts.  A
 * caller that needs the reference's order runs the two stages as two calls: vo_tracker_track with an empty local map
 * (max_local points, n = 0), derives the local map from VO_TRACKER_ASSIGNED_LAST, then vo_tracker_track_local_map.
 * ------------------------------------------------------------------------------------------ */
typedef struct vo_tracker vo_tracker;
typedef struct {
  int32_t batch, width, height;
  int32_t nfeatures, nlevels, ini_th_fast, min_th_fast; /* 0: 1000, 8, 20, 7 (visualOdometry.cpp:31) */
  float scale_factor;                                   /* <= 1: 1.2 */
  float intrinsics[5];                                  /* fx, fy, cx, cy, bf */
  float dist_coef[5];                                   /* k1, k2, p1, p2, k3 */
  int32_t has_distortion;
  float inv_depth_scale;                                /* metres = raw * inv_depth_scale (depth_kind 2) */
  int32_t max_last, max_local;                          /* capacity: last-frame / local map points per frame */
  int32_t max_features;                                 /* feature slots per frame; 0: the extractor's bound */
  int32_t single_stream;
  void *stream, *extract_stream;                        /* hipStream_t or NULL */
  /* relocalisation route (vo_tracker_relocalize): candidate key-frames per frame and features per candidate the tracker
   * can hold; 0 = route unavailable (the config of a caller that does not know these fields) */
  int32_t max_reloc_candidates, max_reloc_features;
} vo_tracker_config;
typedef struct {
  float radius;     /* searchByProjection(frame, last frame): 15 */
  float th_radius;  /* searchByProjection(frame, local points): 3 (5 just after relocalisation, :793-794) */
  float ratio;      /* Matcher(0.8) */
  int32_t direction; /* matcher.cpp:70-75: 0 none, 1 forward, 2 backward */
  float ref_ratio;   /* vo_tracker_track_ref_keyframe: Matcher(0.7) (:262); <= 0: 0.7 */
  int32_t no_retry;  /* 0: a frame with < 20 matches is cleared and searched again at 2 x radius (:241-245), on the
                        device, before the solve; 1: no second search (the status bit still reports < 20) */
} vo_tracker_params;
enum { VO_TRACK_FEW_MATCHES = 1, VO_TRACK_FEW_INLIERS = 2, VO_TRACK_RELOC_FAILED = 4 };
int vo_tracker_create(vo_tracker **out, const vo_tracker_config *cfg);
void vo_tracker_destroy(vo_tracker *t);
int vo_tracker_info(const vo_tracker *t, int *batch, int *max_features, int *max_keypoints, int *n_levels);
vo_orb *vo_tracker_extractor(vo_tracker *t); /* the handles the tracker owns (accessors, tests) */
vo_frames *vo_tracker_frames(vo_tracker *t);
void *vo_tracker_stream(vo_tracker *t);
/* State of the map as the next batch sees it; host arrays [batch][n][...], copied before the call
 * returns.  Last frame (frame_last_->mappoints_, visualOdometry.cpp:232-238): Tcw12 [batch][12] =
 * rotation row-major + translation of frame_curr_->Tcw_ = Tcl_ * frame_last_->Tcw_; per map point its
 * world position, flags (bit 0: exists and is no outlier, bit 1: observe_cnt_ > 0), the octave, angle
 * and descriptor of the last frame's feature.  Local map (localMappoints_, :745-775): world position,
 * normal vector, minDistance_ / maxDistance_ (mappoint.h), flags (bit 0: exists and is not bad, bit 1:
 * observe_cnt_ > 0), descriptor; link[i] = index of the same MapPoint in the last-frame list or -1
 * (NULL: none) -- a point the first search matched carries visualIdxOfFrame_ == frame id and is
 * skipped (:765). */
int vo_tracker_set_last_frame(vo_tracker *t, int n, const double *Tcw12, const double *points, const uint8_t *flags,
                              const int32_t *octave, const float *angle, const uint8_t *desc);
int vo_tracker_set_local_map(vo_tracker *t, int n, const double *points, const double *normals,
                             const float *min_distance, const float *max_distance, const uint8_t *flags,
                             const int32_t *link, const uint8_t *desc);
/* One batch.  _dev: 8-bit grey images [batch] in device memory (row pitch, frame stride in bytes), depth as
 * in vo_frames_build_dev (depth_kind 0 none, 1 float32 metres, 2 uint16 raw).  vo_tracker_track: the same
 * from host memory (width x height, tightly packed; uploads included: the image ahead of the extraction, the depth -- first
 * read by the frame build -- on a copy stream of the tracker behind the extraction's launches.  Page-locked host buffers must
 * stay untouched until vo_tracker_results or a synchronisation; pageable ones are read before the call returns).
 * Asynchronous; params NULL: 15, 3, 0.8, 0. */
int vo_tracker_track_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                         const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                         const vo_tracker_params *params);
int vo_tracker_track(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind,
                     const vo_tracker_params *params);
/* The two stages as two calls (the reference's order: updateLocalKeyFrames / updateLocalMapPoints derive the local map
 * from the matches of the first stage, visualOdometry.cpp:286-291).  vo_tracker_track_first[_dev]: Frame construction,
 * trackWithMotion's search (+ retry), solvePoseOnlySE3, cullingOutliersBeforeLocalMap; vo_tracker_results then returns
 * the first solve's pose, n_tracked = the culling's observed-inlier count (:250), n_inliers = the solve's return value,
 * the status bits of :247 / :253.  vo_tracker_track_local_map: searchLocalMapPoints, solvePoseOnlySE3 and the inlier
 * count on the state the first stage left, against the local map set in between (vo_tracker_set_local_map). */
int vo_tracker_track_first(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind,
                           const vo_tracker_params *params);
int vo_tracker_track_first_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                               const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                               const vo_tracker_params *params);
int vo_tracker_track_local_map(vo_tracker *t, const vo_tracker_params *params);
/* vo_tracker_track_local_map after vo_tracker_relocalize, _store or _db (and their _dev forms): trackLocalMap as the
 * reference runs it behind a successful relocalization() (visualOdometry.cpp:61, :74, :82-83 -> :726-774, :287-310), on the
 * frame state the relocalisation left (VO_TRACKER_FEATURE_HAS_POINT / _POINTS / _OUTLIER, VO_TRACKER_RELOC_POINT_IDS).  The
 * local map is whatever vo_tracker_set_local_map holds -- the caller reads the winners (VO_TRACKER_RELOC_*) and builds it
 * between the two calls -- or what vo_tracker_build_local_map has built on the device; the caller passes th_radius = 5
 * (:768; params NULL: 5, 0.8).  vo_tracker_set_local_map_ids: the map-point id of every local point, ids [batch][n] with n = the local map's n, in the id space VO_TRACKER_RELOC_POINT_IDS reports
 * (the store's global ids after _store / _db, the dense ids after vo_tracker_relocalize; negative: no id).  A local point
 * whose id is held by a non-null, non-outlier slot of its frame is skipped (`mp->visualIdxOfFrame_ == frame id`, :753);
 * the ids belong to the local map they were set for (vo_tracker_set_local_map forgets them), and WITHOUT ids nothing is
 * skipped after a relocalisation (`link` is not used: the frame's points are no entries of a last-frame list).  The
 * search's `occupied` is: the slot holds a point with observations -- bit 1 of the key-frame feature's flags, which the
 * relocalisation routes carry per slot.  The solve runs over all non-null slots, the relocalisation's and the new matches;
 * vo_tracker_results then returns its pose, n_inliers = its return value, n_tracked = inliers_num_ of :289-303 (not
 * outlier, and observed), n_matches_local = the search's count; VO_TRACKER_ASSIGNED_LOCAL its assignment, and
 * VO_TRACKER_RELOC_POINT_IDS includes the new points' ids.  A frame with VO_TRACK_RELOC_FAILED is not touched: every
 * output keeps the value the relocalisation left, n_matches_local 0.  The decision of :307-310 (< 50 right after a
 * relocalisation) is the caller's, from n_tracked.  No local map set, or ids with another n: VO_ERR_INVALID before anything
 * is enqueued.  All enqueued, no synchronisation; on every other route vo_tracker_track_local_map behaves as above. */
int vo_tracker_set_local_map_ids(vo_tracker *t, int n, const int32_t *ids /*[batch][n]*/);
/* VisualOdometry::trackRefKeyFrame (visualOdometry.cpp:256-277) -- the route taken when trackWithMotion fails --
 * followed by trackLocalMap (first_stage_only = 0) or on its own (1): Frame construction, Frame::computeBow (vocabulary
 * transform on the device), Matcher(0.7).searchByBoW(keyframe_trackRef_, frame) (k_node_replay, one workgroup per
 * frame of the batch), `match_num < 15` -> VO_TRACK_FEW_MATCHES, the key-frame's map points into the frame's slots,
 * pose = frame_last_->Tcw_, solvePoseOnlySE3, cullingOutliersBeforeLocalMap.  vo_tracker_set_ref_keyframe: per frame of
 * the batch its reference key-frame's features [batch][n]: the map point of every feature (world position; flags bit 0:
 * exists and is not bad, bit 1: observe_cnt_ > 0), the feature's angle and descriptor, its DBoW3::FeatureVector
 * (nodes[batch], levelsup 3) and Tcw12 [batch][12] = frame_last_->Tcw_.  It REPLACES the last-frame state
 * (vo_tracker_set_last_frame): the key-frame's map points take the place of frame_last_->mappoints_ for the rest of the
 * pipeline (`link` of vo_tracker_set_local_map then indexes the key-frame's features).  The vocabulary must outlive
 * the tracker's use of it.  The common-node walk is host work: this route synchronises once inside the call.
 * vo_tracker_track_ref_keyframe_store below is the same route with the key-frames read from a device store. */
int vo_tracker_set_ref_keyframe(vo_tracker *t, const vo_vocab *vocab, int n, const double *Tcw12, const double *points,
                                const uint8_t *flags, const float *angle, const uint8_t *desc,
                                const vo_bow_view *const *nodes);
int vo_tracker_track_ref_keyframe(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind,
                                  const vo_tracker_params *params, int first_stage_only);
int vo_tracker_track_ref_keyframe_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                                      const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                                      const vo_tracker_params *params, int first_stage_only);
/* VisualOdometry::relocalization() (visualOdometry.cpp:313-395) for every frame of the batch, from Frame construction
 * to the pose.  Per frame and candidate key-frame IN THE CALLER'S ORDER, candidates flagged bad skipped:
 *   Matcher(0.75).searchByBoW(kf, frame); < 15 matches: next.  poseEstimateByPnP (:776-826) = vo_pnp_ransac_dev(100, 8.0,
 *   0.99) on the matches in feature order; its inliers' map points and its pose are written into the frame BEFORE the
 *   `< 10` gate (:336), so a rejected candidate with 1..9 inliers leaves both behind for the next one.
 *   solvePoseOnlySE3 over ALL non-null slots; < 10: next (pose and outliers_ kept, nothing culled).  Outliers culled;
 *   < 50: searchByProjection(frame, kf, 10, 100, found = this candidate's PnP inliers); sum >= 50: solve (NOT culled);
 *   in (30, 50): found = every point in the frame, searchByProjection(frame, kf, 3, 60, found); sum >= 50: solve, cull.
 *   inliers_num_ >= 50: success, the walk stops.
 * MapPoint identity (found.count, the leaked slots) is an int32 id per key-frame feature: the same map point carries
 * the same id in every candidate of a frame; ids lie in [0, max_reloc_candidates x max_reloc_features).
 * vo_tracker_set_reloc_candidates: cands [batch][max_cand] (n_cand[f] <= max_cand of them used per frame), every array
 * copied before the call returns; more candidates or features than configured: VO_ERR_CAPACITY, nothing is truncated.
 * The BoW searches and the PnP of all batch x max_cand pairs run in one pass (they do not depend on the walk); then
 * max_cand rounds of the dependent tail are enqueued unconditionally, round r serving candidate r of every frame still
 * walking.  The common-node walk of searchByBoW is host work: the call synchronises ONCE, after computeBow, and is
 * asynchronous from there.  vo_tracker_results: pose, n_tracked = n_inliers = inliers_num_, status VO_TRACK_RELOC_FAILED
 * when no candidate (or none at all) reached 50; VO_TRACKER_FEATURE_HAS_POINT / _POINTS / _OUTLIER and the
 * VO_TRACKER_RELOC_* selectors describe the frame at the end.  Deviation: the P3P path of solvePnPRansac at exactly 4
 * correspondences (vo_pnp_ransac) cannot occur here (>= 15 matches).
 * On vo_tracker_relocalize_store / vo_tracker_relocalize_db (below) the candidates come from a device store. */
typedef struct {
  int32_t n;                 /* features of the key-frame */
  int32_t bad;               /* KeyFrame::isBad() */
  const float *angle;        /* [n] unKeypoints_[i].angle */
  const uint8_t *desc;       /* [n][32] descriptors_ */
  const vo_bow_view *nodes;  /* featVec_ (levelsup 3) */
  const uint8_t *flags;      /* [n] bit 0: the feature's map point exists and is not bad; bit 1 (key-frame store only):
                                observe_cnt_ > 0 */
  const double *points;      /* [n][3] MapPoint::getPose() */
  const int32_t *ids;        /* [n] map point id */
  const uint8_t *point_desc; /* [n][32] MapPoint::getDescriptor() */
  const float *min_distance, *max_distance; /* [n] minDistance_, maxDistance_ */
} vo_reloc_candidate;
int vo_tracker_set_reloc_candidates(vo_tracker *t, const vo_vocab *vocab, int max_cand, const int32_t *n_cand,
                                    const vo_reloc_candidate *cands);
int vo_tracker_relocalize(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind,
                          const vo_tracker_params *params);
int vo_tracker_relocalize_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                              const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                              const vo_tracker_params *params);

/* The key-frame feature store: everything the relocalisation route reads of a key-frame, resident
 * on the device, so that the route takes its candidates as key-frame numbers.  A key-frame is known by its insertion
 * number 0, 1, 2 ... -- the numbering of vo_kfdb -- and keeps it (vo_kfstore_erase_keyframe marks, it does not reclaim).  Every device buffer is sized at creation from
 * (max_keyframes, max_features); one more key-frame, or a key-frame with more features (or more FeatureVector entries)
 * than that, is VO_ERR_CAPACITY and nothing is truncated.  Per key-frame: n, bad; per feature: angle, desc, flags (bit 0:
 * the map point exists and is not bad; bit 1: observe_cnt_ > 0, the meaning vo_tracker_set_ref_keyframe gives it -- the
 * whole byte is carried by insert, insert_dev and update_points; the relocalisation routes ignore bit 1,
 * vo_tracker_track_ref_keyframe_store reads it), points, ids, point_desc, min / max distance; the FeatureVector (levelsup 3) as a
 * CSR: node ids ascending, start, feat.  ids are global map-point ids: any non-negative int32 (the route maps them to
 * dense ids per frame itself).  Calls on one handle are serialised by the caller; work is enqueued on the handle's stream
 * (NULL, the legacy stream, until vo_kfstore_set_stream).  A tracker call that reads the store orders itself behind
 * that stream with an event, and the store's later work behind the tracker's.
 * insert: vo_reloc_candidate with the validation of vo_tracker_set_reloc_candidates except the id range (ids of flagged
 * features must be >= 0); one staging copy, synchronises the stream once (the caller's arrays are free on return).
 * insert_dev: the arrays in device memory [n], the FeatureVector as the per-feature node id that vo_bow_transform writes:
 * the CSR is built on the device (node ascending, the features of a node in index order: Frame::computeBow's); no host
 * synchronisation, nothing is validated beyond n.  The arrays must stay untouched until the stream has passed the call.
 * set_bad: KeyFrame::isBad() from now on.  update_points: the map side of key-frame `keyframe` replaced (host arrays [n],
 * n as inserted) -- after BA or culling; descriptors, angles and the FeatureVector never change.  Synchronises once. */
typedef struct vo_kfstore vo_kfstore;
int vo_kfstore_create(vo_kfstore **out, int max_keyframes, int max_features);
void vo_kfstore_destroy(vo_kfstore *s);
int vo_kfstore_set_stream(vo_kfstore *s, void *hip_stream);
int vo_kfstore_size(const vo_kfstore *s);
int vo_kfstore_insert(vo_kfstore *s, const vo_reloc_candidate *kf, int32_t *index);
int vo_kfstore_insert_dev(vo_kfstore *s, int n, int bad, const float *dev_angle, const uint8_t *dev_desc,
                          const int32_t *dev_node_of_feature, const uint8_t *dev_flags, const double *dev_points,
                          const int32_t *dev_ids, const uint8_t *dev_point_desc, const float *dev_min_distance,
                          const float *dev_max_distance, int32_t *index);
int vo_kfstore_set_bad(vo_kfstore *s, int keyframe, int bad);
int vo_kfstore_update_points(vo_kfstore *s, int keyframe, const uint8_t *flags, const double *points, const int32_t *ids,
                             const uint8_t *point_desc, const float *min_distance, const float *max_distance);
/* What vo_tracker_build_local_map (below) reads of a key-frame beyond its features.  All three are additive: the records,
 * entry points and results above do not change, and every buffer is sized at creation from (max_keyframes, max_features).
 * set_graph: the covisibility / spanning-tree links VisualOdometry::updateLocalKeyFrames walks (visualOdometry.cpp:649-689).
 * neighbors = getBestCovisibleKFs(10) in its order (n_neighbors <= VO_KFSTORE_MAX_NEIGHBORS); children = getChildren() in
 * ASCENDING KEY-FRAME NUMBER -- the reference's set<KeyFrame*> iterates in pointer order, which no restatement can
 * reproduce: the rule DESIGN.md section 4e states for pointer-keyed containers (a list that is not strictly ascending is
 * VO_ERR_INVALID); at most VO_KFSTORE_MAX_CHILDREN children per key-frame, VO_ERR_CAPACITY beyond (nothing is truncated);
 * parent = getParent() as a key-frame number or -1.  Every id must lie in [0, size), else VO_ERR_INVALID, and nothing
 * changes on an error.  Until set, a key-frame has no neighbours, no children and no parent.  One copy, synchronises once.
 * set_graph_batch: the same for the key-frames first .. first + count - 1 in one call: n_neighbors [count], neighbors
 * [count][VO_KFSTORE_MAX_NEIGHBORS], n_children [count], children [count][VO_KFSTORE_MAX_CHILDREN] (entries beyond the
 * counts are ignored), parent [count]; everything is validated before anything is copied.
 * set_normals: MapPoint::normalVector_ of the key-frame's map points, normals [n][3] (n as inserted), a per-feature column
 * of its own which Frame::isInFrame reads (frame.cpp:176).  THE COLUMN IS ZERO UNTIL SET: a zero normal gives a view
 * cosine of 0 and fails the `cos > 0.5` gate, so a local point built from such a feature is never searched.
 * The observation index (no entry point): map-point id -> the key-frames that hold it, in ascending key-frame number;
 * key-frame k holds id p when one of its features has ids == p and flags bit 0 set.  It stands in for
 * MapPoint::getObservedKFs() and is rebuilt on the device (sorted keys), lazily, by the first
 * vo_tracker_build_local_map after an insert, insert_dev or update_points: launches on the store's stream only, no host
 * synchronisation, no device-to-host copy. */
#define VO_KFSTORE_MAX_NEIGHBORS 10
#define VO_KFSTORE_MAX_CHILDREN 64
int vo_kfstore_set_graph(vo_kfstore *s, int keyframe, int n_neighbors, const int32_t *neighbors, int n_children,
                         const int32_t *children, int parent);
int vo_kfstore_set_graph_batch(vo_kfstore *s, int first, int count, const int32_t *n_neighbors, const int32_t *neighbors,
                               const int32_t *n_children, const int32_t *children, const int32_t *parent);
int vo_kfstore_set_normals(vo_kfstore *s, int keyframe, const double *normals /*[n][3]*/);
/* The covisibility graph and the spanning tree maintained on the device: KeyFrame::updateConnections
 * with addConnection and updateBestCovisibles (keyframe.cpp:69-198), from the observation index, so that insert ->
 * update connections -> vo_tracker_build_local_map -> vo_tracker_track_local_map runs without the host computing anything.
 * enable_connections: valid on an empty store only (size == 0, else VO_ERR_INVALID); allocates the connection state, a dense
 * int32 weight row and an ordered list per key-frame plus five words: 8 * max_keyframes^2 + 20 * max_keyframes + 16 bytes
 * (2 010 016 at 500 key-frames).  max_keyframes above VO_KFSTORE_CONNECTIONS_MAX_KEYFRAMES is VO_ERR_CAPACITY (the count
 * kernel keeps one counter per key-frame in 16 KB of LDS, the order kernel sorts a row in 32 KB; the state would be
 * 128 MB there).  A store without this call allocates and behaves exactly as before.  With it the graph has ONE writer:
 * vo_kfstore_set_graph / _batch return VO_ERR_INVALID.  Synchronises once.
 * update_connections[_dev]: update(k) for every k of the list IN LIST ORDER, repeats allowed; the result is that of the
 * reference called sequentially.  update(k), with "j holds p" as the observation index defines it (the key-frames' bad
 * flag plays no part: updateConnections never tests it):
 *  1 C[j], j != k: the features of k with bit 0 set whose id j holds (:80-93).  An id in two features of k counts twice, j
 *    counts once per feature however many of its features hold the id: C is NOT symmetric.  All zero: nothing changes (:95).
 *  2 nmax / kfmax: the first strictly largest count in ASCENDING KEY-FRAME NUMBER (:105-111; the rule of
 *    vo_kfstore_set_graph for pointer-keyed containers).
 *  3 T = { j : C[j] >= 15 }, or { kfmax } when that is empty (:112-124).
 *  4 addConnection(j <- k, C[j]) for every j of T (:157-171): where the weight j keeps for k is absent or different it is
 *    set and j's ordered list becomes ALL of j's weights, sorted (updateBestCovisibles, :176-198); an equal weight changes
 *    nothing.
 *  5 k's weights become C, every entry >= 1 (:140); k's ordered list is T only, sorted (:127-142).
 *  6 sorted: weight descending, equal weights in DESCENDING key-frame number (sort of (weight, KeyFrame*) pairs ascending,
 *    then push_front).
 *  7 on k's first update that finds a connection, k != 0: parent = the front of k's ordered list, k joins the parent's
 *    children (:145-150).  Key-frame 0 never gets a parent.
 * So a key-frame's ordered list is thresholded right after its own update and becomes its whole weight map, entries below
 * 15 included, as soon as a neighbour's update changes one of its weights -- both visible through getBestCovisibleKFs(10).
 * Besides the state the calls rewrite the graph row (vo_kfstore_set_graph's) of every key-frame whose ordered list, parent
 * or children changed: the first VO_KFSTORE_MAX_NEIGHBORS of the ordered list, the parent, the children ascending;
 * vo_tracker_build_local_map reads it unchanged.  The work runs on the store's stream -- the observation index rebuilt
 * first when an insert or update_points has happened since its last use, then three launches (count, apply, order) -- and
 * tracker calls order themselves behind it like behind any other store call.
 * update_connections: host list; every number is validated against [0, size) before anything is enqueued (VO_ERR_INVALID,
 * nothing changes); one copy, synchronises once (the list is free on return).
 * update_connections_dev: device list [n], which must stay untouched until the stream has passed the call.  Enqueues only: no
 * host synchronisation, no device-to-host copy, no allocation except by the first call with a larger n than any before.
 * Conditions only the device sees go to a sticky word on the store: a listed number outside [0, size) is skipped
 * (VO_KFSTORE_CONNECTIONS_INVALID); a parent with more than VO_KFSTORE_MAX_CHILDREN children keeps its 64 lowest-numbered
 * ones in its graph row (VO_KFSTORE_CONNECTIONS_CAPACITY; the child's parent is still set).
 * connections_status: synchronises, returns the word and clears it.
 * get_connections: synchronises; any pointer may be NULL.  n_connected and weights [size] = connectedKFWts_ (0: not
 * connected); n_ordered, ordered [size], ordered_weights [size] = orderedConnectKFs_ / orderedWTs_ (entries beyond
 * n_ordered: -1 / 0); parent = getParent() or -1; n_children, children [VO_KFSTORE_MAX_CHILDREN] = the graph row's
 * (entries beyond n_children: -1).
 * A store with culling (below) skips a listed key-frame that has been erased like a number outside the store.
 * Loop edges: vo_kfstore_add_loop_edge below, on a store with that block. */
#define VO_KFSTORE_CONNECTIONS_MAX_KEYFRAMES 4096
#define VO_KFSTORE_CONNECTIONS_INVALID 1
#define VO_KFSTORE_CONNECTIONS_CAPACITY 2
int vo_kfstore_enable_connections(vo_kfstore *s);
int vo_kfstore_update_connections(vo_kfstore *s, int n, const int32_t *keyframes);
int vo_kfstore_update_connections_dev(vo_kfstore *s, int n, const int32_t *dev_keyframes);
int vo_kfstore_connections_status(vo_kfstore *s, int32_t *word);
int vo_kfstore_get_connections(vo_kfstore *s, int keyframe, int32_t *n_connected, int32_t *weights, int32_t *n_ordered,
                               int32_t *ordered, int32_t *ordered_weights, int32_t *parent, int32_t *n_children, int32_t *children);
/* Redundant key-frames culled on the device: LocalMapping::cullingKeyFrames (localMapping.cpp:434-494)
 * with KeyFrame::eraseKeyFrame, eraseConnection (keyframe.cpp:400-526) and MapPoint::eraseObservedKF / eraseMapPoint
 * (mappoint.cpp:333-381), on the observation index and the connection state, so that a store with device-side connections
 * can lose a key-frame without the host computing or uploading anything.  A store that does not call enable_culling
 * allocates and behaves exactly as before; every entry point of this block except get_flags returns VO_ERR_INVALID on it.
 * enable_culling: valid only on an EMPTY store on which vo_kfstore_enable_connections has succeeded, else VO_ERR_INVALID.
 * Allocates three per-feature columns [max_keyframes][max_features] -- octave (int32, default 0), depth and u_right (float,
 * default -1: what Frame::findDepth gives a feature without depth, frame.cpp:113-131) -- and seven words per key-frame
 * (erased, locked, pending, and the four-word record of the last cull call): 12 * max_keyframes * max_features +
 * 28 * max_keyframes + 16 bytes (6 014 016 at 500 key-frames of 1000 features).  A key-frame whose columns were never set has
 * mp_cnt == 0 and is never culled.  Synchronises once.
 * set_keypoints: host arrays [n], n as inserted; one copy, synchronises once.  set_keypoints_dev: device arrays [n],
 * enqueues only (for insert_dev callers); the arrays must stay untouched until the stream has passed the call.  Both
 * validate the key-frame number against [0, size).
 * set_erase_lock: notEraseLoopDetecting_ (keyframe.cpp:408-412, 541-560) of a key-frame, on or off; enqueues only.  Taking the
 * lock off erases nothing: the caller reads `pending` (cull_state) and calls erase_keyframe, which is
 * setEraseLoopDetectingKF's second half.  Loop edges themselves are the caller's.
 * Definitions (choices of this restatement):
 *  - key-frame j HOLDS id p when one of its features has ids == p and flags bit 0 set and j is not erased;
 *  - j's OBSERVATION of p is its lowest-numbered such feature (observedKFs_ has one entry per key-frame, addObservation
 *    keeps the first: mappoint.cpp:52-58);
 *  - obs(p) = the sum over the holders of 2 where u_right >= 0 at the observation, else 1 (mappoint.cpp:60-63);
 *  - bad(j) = the record's bad flag (vo_kfstore_set_bad and the erase write it).
 * cull_keyframes(current, th_depth), the result being that of the reference called once:
 *  1 the candidates are current's ordered list as the call finds it (:439 copies it), walked in its order; a candidate
 *    with bad(k) or k == 0 is skipped (:445).
 *  2 every feature i of k with bit 0 set: skipped when depth[i] < 0 || depth[i] > th_depth (float comparison, :455); else
 *    mp_cnt++, and when obs(id) > 3, the holders j != k with !bad(j) whose observation has octave <= octave[i] + 1 are
 *    counted: three or more give re_obs++ (:460-483).  An id in two features of k counts once per feature, each with its
 *    own octave.
 *  3 k is erased when re_obs > 0.9 * mp_cnt (:487; in double as written -- for every count a store can hold the product
 *    decides like 10 * re_obs > 9 * mp_cnt, so a tie keeps k and mp_cnt == 0 never erases).  An erase changes what every later
 *    candidate of the call sees.
 * erase(k), also the explicit call erase_keyframe:
 *  - k == 0 or k already erased: nothing happens.  locked[k]: pending[k] = 1 and nothing else (the cull reports decision 2).
 *  - for every j with W[k][j] != 0: where W[j][k] != 0 it becomes 0 and j's ordered list becomes its whole map
 *    (eraseConnection + updateBestCovisibles).  QUIRK Q-E1: the walk runs over k's map, not over who points at k, so a j with
 *    W[j][k] != 0 but W[k][j] == 0 keeps its connection to the erased k (keyframe.cpp:415-416).
 *  - for every observation of k: k leaves the holders; when the remaining obs(p) <= 2 the point dies (eraseMapPoint): bit 0 is
 *    cleared in every feature that carries p of every key-frame not erased before, and of k itself.  Weights do not change
 *    with a point's death.
 *  - W[k][*] = 0 and k's ordered list is empty.
 *  - spanning tree (:429-485): the candidate set starts as {parent[k]} (empty when k has no parent: the reference dereferences
 *    null there).  A round takes, over the non-bad children c of k in ascending number and the members x of c's ordered list
 *    that are in the set, the strictly largest W[c][x] -- ties: the first c, then the first x in list order, i.e. the higher
 *    number --, sets parent[c] = x and moves c from the children into the set; rounds repeat until one finds nothing.  The
 *    remaining children, bad ones included, get parent[k].  k leaves its parent's children; parent[k] itself is KEPT (the
 *    caller's Tcp_; the store holds no poses).
 *  - erased[k] = 1 and the record's bad flag is set.  The slot is not reclaimed.
 * Afterwards the observation index skips erased key-frames (so do vo_tracker_build_local_map's votes), a parent's children
 * are the non-erased key-frames whose parent it is, an erased key-frame's graph row is empty with its parent kept, and
 * update_connections skips a listed erased key-frame (VO_KFSTORE_CONNECTIONS_INVALID).  More than VO_KFSTORE_MAX_CHILDREN
 * children after a re-parenting: VO_KFSTORE_CONNECTIONS_CAPACITY as before.  Map::eraseKeyFrame (map.cpp:37-58) edits a copy
 * of each inverted-index list: vo_kfdb needs nothing.
 * cull_keyframes / erase_keyframe validate the number against [0, size) and ENQUEUE ONLY on the store's stream: the index
 * rebuilt first when stale, then count, apply and the ordering pass (erase_keyframe: apply and order).  No host
 * synchronisation, no device-to-host copy, no allocation.  Every such call marks the index stale (the host cannot know
 * whether anything was erased).  That `current` has been erased only the device knows: the call then walks no candidate
 * and raises VO_KFSTORE_CONNECTIONS_INVALID.
 * cull_result: synchronises; the record of the last cull call: n_candidates and, per candidate in list order, the key-frame,
 * mp_cnt, re_obs (0 / 0 for a skipped one) and decision (arrays [size], any may be NULL).  cull_state: synchronises; any
 * pointer may be NULL.  get_flags: synchronises; the flags bytes [n] and the bad flag of a key-frame as the store holds them
 * (valid on every store). */
#define VO_KFSTORE_CULL_KEPT 0
#define VO_KFSTORE_CULL_ERASED 1
#define VO_KFSTORE_CULL_PENDING 2
#define VO_KFSTORE_CULL_SKIPPED 3
int vo_kfstore_enable_culling(vo_kfstore *s);
int vo_kfstore_set_keypoints(vo_kfstore *s, int keyframe, const int32_t *octave, const float *depth, const float *u_right);
int vo_kfstore_set_keypoints_dev(vo_kfstore *s, int keyframe, const int32_t *dev_octave, const float *dev_depth,
                                 const float *dev_u_right);
int vo_kfstore_set_erase_lock(vo_kfstore *s, int keyframe, int on);
int vo_kfstore_cull_keyframes(vo_kfstore *s, int current, float th_depth);
int vo_kfstore_erase_keyframe(vo_kfstore *s, int keyframe);
int vo_kfstore_cull_result(vo_kfstore *s, int32_t *n_candidates, int32_t *keyframes, int32_t *mp_cnt, int32_t *re_obs,
                           int32_t *decision);
int vo_kfstore_cull_state(vo_kfstore *s, int keyframe, int32_t *erased, int32_t *locked, int32_t *pending);
int vo_kfstore_get_flags(vo_kfstore *s, int keyframe, uint8_t *flags, int32_t *bad);
/* New map points created on the device: LocalMapping::createNewMapPoints (localMapping.cpp:132-361)
 * with computeF12 (:526-536), Matcher::searchForTriangulation (matcher.cpp:867-1010) and the MapPoint constructor,
 * addObservation, computeDescriptor and updateNormalAndDepth (mappoint.cpp:36-179) for a point with two holders, so that a
 * store carries insert -> connections -> new points -> local map -> cull without the host computing anything.  A store
 * that does not call enable_mapping allocates and behaves exactly as before; every entry point of this block except
 * get_points returns VO_ERR_INVALID on it.
 * enable_mapping: valid only on an EMPTY store on which vo_kfstore_enable_culling has succeeded (the step reads octave,
 * depth, u_right, erased and the graph row), else VO_ERR_INVALID.  cam = fx, fy, cx, cy, bf, b as the floats Camera holds
 * (b_ = bf_ / fx_ is the caller's); 1 <= n_levels <= 16 with scale_factors = scaleFactors_; first_point_id >= 0 = the first
 * id the store hands out (MapPoint::factory_id_).  max_features above 16384 is VO_ERR_CAPACITY (k_node_replay's LDS).
 * Allocates, with K = max_keyframes, N = max_features and every array rounded up to 16 bytes: Tcw per key-frame as 12
 * doubles (R row-major, then t; zero until set) with the pose-set word in a thirteenth slot (104 K); unKeypoints_[i].pt per
 * feature as two float columns, a key-frame's side by side (8 K N); the id counter (16); the result record (176) and its created rows (160 N); the scratch of ONE neighbour
 * step -- query list and claims (32 N), claimable bytes (N), match12 (4 N), the argument block (304), the match count (16),
 * the step's geometry (336): 8 K N + 104 K + 197 N + 848 bytes as listed, 4 249 848 at 500 key-frames of 1000 features,
 * and 4 249 856 allocated there (the rounding adds 8 to the claimable bytes).  Synchronises once.
 * set_pose: Tcw12 = R row-major then t (host, doubles); one copy, synchronises once.  set_pose_dev: the same from device
 * memory, enqueues only.  set_keypoint_xy: xy [n][2] (host, floats; n as inserted) = unKeypoints_[i].pt; one copy,
 * synchronises once.  set_keypoint_xy_dev: device array, enqueues only; it must stay untouched until the stream has passed
 * the call.  All four validate the key-frame number against [0, size).  next_point_id: synchronises; the id the next
 * created point gets.
 * create_map_points(current, max_neighbors): current in [0, size) and max_neighbors in [1, 10] are validated (the
 * reference leaves after the first neighbour when key-frames are waiting, :163: the caller says which case holds);
 * everything else is ENQUEUED on the store's stream: no host synchronisation, no device-to-host copy, no allocation;
 * three launches per neighbour step, 3 * max_neighbors per call.  The result is that of the reference called once:
 *  1 neighbours: the first max_neighbors entries of current's graph row (getBestCovisibleKFs(10), copied at :136) as the
 *    call finds them, in order.  bad(kf): skipped (:167).  (float)|Owi - Owc| < b: skipped (:172-174).  A neighbour without a
 *    pose: skipped, and the sticky VO_KFSTORE_CONNECTIONS_INVALID is raised.  current erased or without a pose: the call
 *    creates nothing, the record is empty and the same bit is raised.
 *  2 per neighbour, in double with every operation rounded on its own, in the order DESIGN.md section 4j writes down:
 *    Ow = -R^T t, R12 = R1 R2^T, t12 = t1 - R12 t2, F12 = K^-T [t12]x R12 K^-1 in closed form, and the epipole
 *    camera2pixel(R2 Ow1 + t2) rounded to float (matcher.cpp:887-891).
 *  3 searchForTriangulation(current, kf, F12, checkRot = true), bit-exact as vo_match_triangulation is; both FeatureVectors
 *    are the store's; "has a map point" is flags bit 0 AS THE STEP FINDS IT (the reference tests the pointer, which is
 *    non-null for a bad point too: the store folds "exists and is not bad" into bit 0 -- a choice of this restatement), so a
 *    feature neighbour i received a point for is out of neighbour i + 1's search, claims nothing there and enters no
 *    rotation histogram: what vo_match_triangulation_batch, whose searches are independent, cannot give.
 *  4 per match (idx1, idx2) in ascending idx1 (:192-341): pcam through the float pixel2camera(kp, 1); cosParallaxRay in
 *    double rounded to float; cosParallaxDepth1 when stereo1, cosParallaxDepth2 ONLY when !stereo1 && stereo2 (the
 *    `else if` of :222 -- a quirk, reproduced); the point from the linear triangulation (vo_triangulate's arithmetic,
 *    |x3| < 1e-8 skips), else key-point 1 back-projected at depth1, else key-point 2 at depth2, else the match is skipped;
 *    z1 <= 0 and z2 <= 0 reject; the float reprojection gates 5.991 (no u_right) and 7.815 (with the u - bf / z term) over
 *    scaleFactors[octave]^2; a distance below 1e-6 rejects; the scale-consistency gate with 1.5f * scaleFactors[1].
 *  5 commit (:344-355): the id from the counter in creation order (neighbour order, then ascending idx1); into feature idx1
 *    of current and idx2 of the neighbour: flags = 3 (bit 0 | bit 1), the id, the point (the float SVD result widened, or
 *    the back-projection's doubles), point_desc = the descriptor of the LOWER-NUMBERED of the two key-frames
 *    (computeDescriptor with two holders: both medians are 0 and the test is strict), min / max distance
 *    (max = (float)|p - Owc| * scaleFactors[octave[idx1]], min = max / scaleFactors[n_levels - 1]) and, in the normals
 *    column, the mean of the two unit vectors (p - Ow) / |p - Ow|.  Connection weights do not change (the reference does
 *    not call updateConnections here).  The observation index is marked stale.
 * new_points_result: synchronises; the record of the last call.  n_neighbors = the entries of current's row the call
 * saw (at most 10); per entry the key-frame, a status (entries beyond max_neighbors: NOT_REACHED), the search's match_cnt
 * and the number of points created (arrays [10], any may be NULL); created [sum][4] = (key-frame of the neighbour, idx1,
 * idx2, id) per new point in creation order, at most created_capacity rows (the record holds 10 * max_features).  Returns
 * VO_ERR_CAPACITY, with everything else filled in, when the call created more rows than created_capacity.
 * get_points: synchronises; the map side of a key-frame as the store holds it, arrays [n] (n as inserted), any may be
 * NULL: flags, ids, points [n][3], point_desc [n][32], min / max distance, normals [n][3].  Valid on every store. */
#define VO_KFSTORE_NP_SEARCHED 0
#define VO_KFSTORE_NP_SKIPPED_BAD 1
#define VO_KFSTORE_NP_SKIPPED_BASELINE 2
#define VO_KFSTORE_NP_SKIPPED_NO_POSE 3
#define VO_KFSTORE_NP_NOT_REACHED 4
int vo_kfstore_enable_mapping(vo_kfstore *s, const float cam[6], int n_levels, const float *scale_factors, int32_t first_point_id);
int vo_kfstore_set_pose(vo_kfstore *s, int keyframe, const double *Tcw12);
int vo_kfstore_set_pose_dev(vo_kfstore *s, int keyframe, const double *dev_Tcw12);
int vo_kfstore_set_keypoint_xy(vo_kfstore *s, int keyframe, const float *xy /*[n][2]*/);
int vo_kfstore_set_keypoint_xy_dev(vo_kfstore *s, int keyframe, const float *dev_xy /*[n][2]*/);
int vo_kfstore_next_point_id(vo_kfstore *s, int32_t *id);
int vo_kfstore_create_map_points(vo_kfstore *s, int current, int max_neighbors);
int vo_kfstore_new_points_result(vo_kfstore *s, int32_t *n_neighbors, int32_t *neighbor_kf /*[10]*/, int32_t *status /*[10]*/,
                                 int32_t *n_matches /*[10]*/, int32_t *n_created /*[10]*/, int32_t *created /*[sum][4]*/,
                                 int created_capacity);
int vo_kfstore_get_points(vo_kfstore *s, int keyframe, uint8_t *flags, int32_t *ids, double *points, uint8_t *point_desc,
                          float *min_distance, float *max_distance, double *normals);
/* Local bundle adjustment from the store: Optimizer::solveLocalBAPoseAndPoint
 * (optimizer_ceres.cpp:446-808) with the window gathered (:449-592) and the result written back (:757-804) on the device,
 * MapPoint::eraseObservedKF / eraseMapPoint (mappoint.cpp:333-381) and MapPoint::updateNormalAndDepth (mappoint.cpp:66-116)
 * included; the solve in between is vo_ba's, unchanged.  A store that does not call enable_local_ba allocates and behaves
 * exactly as before; every entry point of this block returns VO_ERR_INVALID on it.  "holds", "observation", obs(p) and bad(j)
 * are section 4i's definitions above; pointer-keyed containers are walked in ascending key-frame number.
 * enable_local_ba(max_cams, max_points, max_edges): valid only on an EMPTY store on which vo_kfstore_enable_mapping has
 * succeeded, else VO_ERR_INVALID; capacities below 1 are VO_ERR_INVALID.  Allocates, with K = max_keyframes, N =
 * max_features, C / P / E the capacities and every array rounded up to 16 bytes: ref_kf = MapPoint::keyFrame_ref_ per
 * feature (int32, default -1: unknown; 4 K N); three words per key-frame (12 K); the point grid's workgroup counts
 * (4 ceil(K N / 256)); per point the edge offsets, refresh_points' list and the dead byte (9 P + 4); the window -- the
 * record (64), cameras (53 C), points (28 P), edges (44 E); the apply's inputs (96 C + 24 P + E): 4 K N + 4 ceil(K N / 256) +
 * 12 K + 149 C + 61 P + 45 E + 68 bytes as listed, 5 472 252 at 500 key-frames of 1000 features with 64 cameras, 8192 points
 * and 65536 edges, and 5 472 272 allocated there; and ONE page-locked staging block of the larger of the window and the inputs
 * (host memory, 3 116 416 bytes there, before the allocator's headroom).  Synchronises once.
 * set_point_refs: ref_kf [n] (host, n as inserted) of a key-frame's features; values in [-1, size), else VO_ERR_INVALID; one
 * copy, synchronises once.  set_point_refs_dev: device array [n], enqueues only, not validated (a value outside the holders
 * resolves like -1); it must stay untouched until the stream has passed the call.  create_map_points writes ref_kf = current
 * into both features of a point it creates (mappoint.cpp:37).  An erase (section 4i) leaves the column alone: a reference
 * key-frame that no longer holds the point is resolved by the next refresh (mappoint.cpp:350-351).
 * local_ba_window(current): current in [0, size) is validated; everything else is ENQUEUED on the store's stream -- the index
 * rebuilt first when stale, then five launches; no host synchronisation, no device-to-host copy, no allocation.  The window
 * is that of the reference called once:
 *  1 cameras: camera 0 is current; then current's WHOLE ordered list (getOrderedKFs(): vo_kfstore_get_connections' `ordered`,
 *    not the ten-entry graph row) as the call finds it, in its order, entries with bad(j) skipped (:461).  A skipped entry is
 *    still marked local (:459 comes before the test) and never becomes a fixed camera.
 *  2 points: the local cameras in list order, their features ascending, bit 0 set: the FIRST occurrence of an id is point j,
 *    its position the store's row at that occurrence (:480-499).
 *  3 fixed cameras: every key-frame with !bad that holds a local point and is neither current nor in the ordered list,
 *    appended in ascending key-frame number (:502-528).  cam_fixed = fixed, or the key-frame is number 0 (:578).
 *  4 edges: points in order, per point its holders in ascending key-frame number, each at its observation: camera, point
 *    and feature index, obs = (x, y, u_right) widened to double, inv_sigma = 1.0 / (double)scale_factors[octave] (:555-591).
 *    A holder without a camera -- a bad one, in the list or not -- gets no edge and is counted in n_dropped (the reference
 *    dereferences a null pose block there, :561).
 *  5 poses6 = [upsilon; omega] of Tcw through vo_se3_log's arithmetic.
 *  6 current erased or without a pose, or any camera without a pose: the window is EMPTY (all counts 0) and the sticky
 *    VO_KFSTORE_CONNECTIONS_INVALID is raised.  More cameras, points or edges than the capacities: the window is OVERFLOWED,
 *    the sticky VO_KFSTORE_LOCAL_BA_CAPACITY is raised (vo_kfstore_connections_status reads and clears both), the record
 *    holds the TRUE counts and no array is valid; nothing is truncated.
 * local_ba_window_result: synchronises (one copy into the staging block); record [16] = n_cams, n_local (current and the
 * list's cameras), n_fixed, n_points, n_edges, n_dropped, status (VO_KFSTORE_BA_WINDOW_*), current, and of the last apply
 * n_erased, n_feature0, n_dead; five zeros.  Arrays sized by the capacities, filled to the counts when the status is OK: cam_keyframe,
 * cam_fixed, poses6 [n_cams][6], point_id, points [n_points][3], edge_cam, edge_point, edge_feature, edge_obs [n_edges][3],
 * edge_inv_sigma.  Any pointer may be NULL.
 * local_ba_apply(poses6, points, edge_erase): a solver's result for the LAST window, host arrays in the window's order
 * ([n_cams][6], [n_points][3], [n_edges]); one copy out of the staging block, two launches, one synchronisation at the end
 * (the staging block is free on return).  VO_ERR_INVALID when there
 * is no window, the last one is empty or overflowed, or the store has been changed since (every call of this header that
 * writes the store, an apply included, advances a generation word; reads do not).  The record is fetched first when no
 * local_ba_window_result has done so (one synchronisation).  In the reference's order:
 *  a erased edges (k, p): k leaves the holders of p -- bit 0 is cleared in EVERY feature of k that carries p.  The store has
 *    one fact where the reference has two (mappoints_[idx] and observedKFs_), so quirk Q-B3 (`if (idx > 0)` at :768 leaves
 *    feature 0 pointing at a point that no longer lists the key-frame) cannot be stored: n_feature0 counts the erased edges
 *    whose observation is feature 0, for a caller that keeps the pointer model; and a second feature of k that carries p does
 *    not turn k back into a holder.
 *  b a point with an erased edge whose remaining obs(p) <= 2 dies (mappoint.cpp:353-381): bit 0 is cleared in every
 *    feature that carries it.  The order of the erases does not matter: obs only falls.
 *  c free cameras get SE3::exp(poses6) -- vo_se3_exp, evaluated on the host while staging -- as Tcw12 in the pose column;
 *    fixed cameras keep their bytes.
 *  d the new position of p goes to every live feature that carries p, in every key-frame; then p is refreshed (below) on the
 *    poses of c and the holders of a / b.  Dead points are not refreshed; rows of cleared features keep their bytes.
 *  e the index is marked stale.  Connection weights do not change.
 * refresh_points(n, ids): MapPoint::updateNormalAndDepth for a host list of ids (n <= max_points, else VO_ERR_CAPACITY; ids
 * >= 0); one copy, synchronises once (the list is free on return), the index rebuilt first when stale, one launch.  Per id:
 *  - its holders in ascending key-frame number, bad ones INCLUDED (:93-100 do not test isBad); a holder without a pose is left
 *    out of the sum and raises the sticky VO_KFSTORE_CONNECTIONS_INVALID;
 *  - ref(p) = ref_kf at p's first live key, or, when that is -1 or no longer a holder, the lowest-numbered holder; the
 *    resolved value is written to every live feature that carries p;
 *  - in double, every operation rounded on its own (DESIGN.md section 4k has the order): Ow = -(R^T t) as in section 4j,
 *    d = p - Ow, normal = (sum over the holders of d / |d|) / n; max = (float)|p - Ow_ref| * scale_factors[octave at ref's
 *    observation], min = max / scale_factors[n_levels - 1] in float;
 *  - the normal and min / max go to every live feature that carries p (no holder has a pose: the normal stays; ref has none:
 *    min / max stay).
 * local_ba(ba, current, stop, summaries): window, ONE device-to-host copy into the staging block, vo_ba_reset(ba, ...) +
 * vo_ba_local_ba(ba, stop, ...) on the CALLER's handle (one per thread, any previous problem is replaced; cam = the store's
 * fx, fy, cx, cy, bf widened), apply.  VO_ERR_STOPPED as vo_ba_local_ba returns it (the reference's return at :594): nothing
 * is written back.  VO_ERR_CAPACITY for an overflowed window, VO_ERR_INVALID for an empty one, and whatever vo_ba_reset
 * refuses: nothing is written back.  summaries: NULL or [2].  `map_->getAllKeyFramesCnt() > 2` stays the caller's test.
 * (Declared behind vo_ba below.)
 * get_point_refs / get_pose: synchronise; the ref_kf column [n] of a key-frame, and its Tcw12 with the pose-set word, as the
 * store holds them (get_pose: valid on every store with mapping). */
#define VO_KFSTORE_LOCAL_BA_CAPACITY 4
#define VO_KFSTORE_BA_WINDOW_OK 0
#define VO_KFSTORE_BA_WINDOW_EMPTY 1
#define VO_KFSTORE_BA_WINDOW_OVERFLOW 2
int vo_kfstore_enable_local_ba(vo_kfstore *s, int max_cams, int max_points, int max_edges);
int vo_kfstore_set_point_refs(vo_kfstore *s, int keyframe, const int32_t *ref_kf);
int vo_kfstore_set_point_refs_dev(vo_kfstore *s, int keyframe, const int32_t *dev_ref_kf);
int vo_kfstore_get_point_refs(vo_kfstore *s, int keyframe, int32_t *ref_kf);
int vo_kfstore_local_ba_window(vo_kfstore *s, int current);
int vo_kfstore_local_ba_window_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *cam_keyframe, uint8_t *cam_fixed,
                                      double *poses6, int32_t *point_id, double *points, int32_t *edge_cam, int32_t *edge_point,
                                      int32_t *edge_feature, double *edge_obs, double *edge_inv_sigma);
int vo_kfstore_local_ba_apply(vo_kfstore *s, const double *poses6, const double *points, const uint8_t *edge_erase);
int vo_kfstore_refresh_points(vo_kfstore *s, int n, const int32_t *ids);
int vo_kfstore_get_pose(vo_kfstore *s, int keyframe, double *Tcw12, int32_t *pose_set);
/* Map-point upkeep on the device: the two steps that open every iteration of LocalMapping::run --
 * processNewKeyFrame (localMapping.cpp:100-130) and cullingMapPoints (:496-524) -- with MapPoint::computeDescriptor
 * (mappoint.cpp:118-179) and eraseMapPoint (:362-381), for a caller who inserts with vo_kfstore_insert_dev and keeps no host
 * copy of ids or flags.  Opt-in and additive: a store without it allocates and behaves as before.  The definitions are section
 * 4i's (j HOLDS p, j's OBSERVATION of p, obs(p), bad(j)).
 * enable_point_upkeep(max_recent): valid on an EMPTY store on which vo_kfstore_enable_local_ba has succeeded (the steps use
 * ref_kf and the refresh), max_recent >= 1; anything else VO_ERR_INVALID.  One device block of
 *   16 + 6 * up16(4 R) + 64 + up16(12 (R + NK)) + up16(4 (R + NK)) + up16(4 NK)   bytes, R = max_recent, NK = max_features,
 *   up16(x) = x rounded up to 16:
 * the head words; the RECENT LIST, addedMapPoints_ (:355, :124) -- id, first_kf (firstAddedIdxofKF_ as a key-frame number),
 * found, visible (found_cnt_, visible_cnt_; int32) per entry, at most R entries; the record of the last upkeep call (16 ints)
 * with its erased ids (R) and a cull call's branch per entry (R); and the scratch: a call's id list with its two counter
 * columns (3 (R + NK)), the overflow list of compute_descriptors (R + NK), process_new_keyframe's candidates (NK).  No
 * per-point outcome depends on the order of the list; the getter reports ascending id.  Synchronises once.
 * compute_descriptors(n, ids): a host list, n <= max_recent + max_features (else VO_ERR_CAPACITY), ids >= 0 (else
 * VO_ERR_INVALID); one copy, one synchronisation at the end.  compute_descriptors_dev(n, dev_ids): the same bound on n; a
 * negative id is skipped; ENQUEUED only -- the index rebuilt first when stale, a 4-byte memset and two launches; no host
 * synchronisation, no device-to-host copy, no allocation; the list must stay untouched until the stream has passed the call.
 * Per id p: desp = the `desc` rows of p's holders in ascending key-frame number, each at its observation, holders with
 * bad(j) left out (:138).  desp empty (no holder, or every holder bad): nothing changes (:131, :142).  Otherwise the winner
 * is the FIRST row with the strictly smallest median, the median being entry int(0.5 * (N - 1)) of the sorted row of Hamming
 * distances, diagonal 0 included (:160-173; vo_median_descriptor's rule).  Its 32 bytes go to point_desc of every live
 * feature that carries p, in every non-erased key-frame (bad ones included), as vo_kfstore_refresh_points writes normals.
 * Repeated ids give the same bytes.  A point with more than VO_KFSTORE_DESC_MAX_HOLDERS non-bad holders keeps its descriptor
 * and raises the sticky VO_KFSTORE_UPKEEP_CAPACITY (read and cleared by vo_kfstore_connections_status).
 * process_new_keyframe(current): for the key-frame just inserted (computeBow, :108, and map_->insertKeyFrame, :129, are the
 * insert).  current in [0, size) is validated; the rest is ENQUEUED (index rebuild when stale, classify, refresh, descriptors,
 * append, vo_kfstore_update_connections_dev's launches for `current`, :128): no host synchronisation, no copy back, no
 * allocation.  current erased: nothing changes, the sticky VO_KFSTORE_CONNECTIONS_INVALID is raised.  Every id p that current
 * holds is handled once, at current's observation of it:
 *  - TRACKED, another non-erased key-frame holds p (the !beObserved branch, :116-121; the store has one fact where the
 *    reference has mappoints_[i] and observedKFs_, so addObservation is the insert): p is refreshed as by
 *    vo_kfstore_refresh_points and gets compute_descriptors, over its holders, current included;
 *  - CREATED WITH THE KEY-FRAME, only current holds p (createNewKeyFrame's stereo points, visualOdometry.cpp:496-503): p is
 *    appended to the recent list with first_kf = current, found = visible = 1 (mappoint.cpp:38-41), unless listed already
 *    (the call is idempotent).
 *  The split by holders is this restatement's; it differs from a pointer model for a tracked point whose other holders have
 *  all been erased (here: created-with).  If the appends would exceed max_recent NONE is made, VO_KFSTORE_UPKEEP_CAPACITY is
 *  raised, the record holds the true count, and the refreshes and the connection update still happen.
 * vo_kfstore_create_map_points on a store with upkeep enqueues one more launch: the ids of its created rows are appended
 * (addedMapPoints_.push_back, :355) with first_kf = current, found = visible = 1, under the same capacity rule.
 * add_point_stats(n, ids, visible, found): host lists, n <= max_recent + max_features, increments >= 0 (else VO_ERR_INVALID);
 * one copy, one synchronisation.  add_point_stats_dev: ENQUEUED only (one launch).  visible[i] / found[i] are added to the
 * entry of ids[i]; a negative id is skipped, an id without an entry ignored (getFoundRatio's only caller is :509), repeats
 * accumulate.
 * cull_map_points(current): current in [0, size) validated; ENQUEUED (index rebuild when stale, two launches).  Per entry, in
 * the reference's branch order:
 *  1 no non-erased key-frame holds the id (isBad()): the entry leaves the list;
 *  2 (float)found / (float)visible < 0.25f (a correctly rounded float division, compared in float): eraseMapPoint, leaves;
 *  3 current > first_kf + 2 && obs(p) <= 3: eraseMapPoint, leaves;
 *  4 current > first_kf + 3: leaves, the point lives;
 *  5 otherwise the entry stays.
 * eraseMapPoint clears bit 0 in EVERY feature that carries the id, in every non-erased key-frame; rows keep their other
 * bytes; connection weights do not change.  Afterwards the index is stale and the generation word has advanced.
 * recent_points(n, ids, first_kf, found, visible) and upkeep_result(record, erased_ids) synchronise; any pointer may be NULL;
 * arrays of max_recent entries.  record [16] = kind (VO_KFSTORE_UPKEEP_*), current, n_tracked, n_new (the appends the call
 * wanted), n_appended, then of a cull call the counts of branches 1 .. 5 and n_erased (branches 2 + 3, the length of
 * erased_ids, ascending), the list's length after the call, four zeros. */
#define VO_KFSTORE_UPKEEP_CAPACITY 8
#define VO_KFSTORE_DESC_MAX_HOLDERS 1024
#define VO_KFSTORE_UPKEEP_PROCESS 1
#define VO_KFSTORE_UPKEEP_CULL 2
#define VO_KFSTORE_UPKEEP_CREATED 3
int vo_kfstore_enable_point_upkeep(vo_kfstore *s, int max_recent);
int vo_kfstore_compute_descriptors(vo_kfstore *s, int n, const int32_t *ids);
int vo_kfstore_compute_descriptors_dev(vo_kfstore *s, int n, const int32_t *dev_ids);
int vo_kfstore_process_new_keyframe(vo_kfstore *s, int current);
int vo_kfstore_add_point_stats(vo_kfstore *s, int n, const int32_t *ids, const int32_t *visible, const int32_t *found);
int vo_kfstore_add_point_stats_dev(vo_kfstore *s, int n, const int32_t *dev_ids, const int32_t *dev_visible, const int32_t *dev_found);
int vo_kfstore_cull_map_points(vo_kfstore *s, int current);
int vo_kfstore_recent_points(vo_kfstore *s, int32_t *n, int32_t *ids, int32_t *first_kf, int32_t *found, int32_t *visible);
int vo_kfstore_upkeep_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *erased_ids);
/* Map-point fusion on the device: LocalMapping::searchInNeighbors (localMapping.cpp:363-432) with
 * Matcher::fuseMapPoints (matcher.cpp:1012-1133) and MapPoint::replaceMapPoint (mappoint.cpp:214-253) on the store.  Opt-in
 * and additive: a store without it allocates and behaves as before.  The definitions are section 4i's (j HOLDS p, j's
 * OBSERVATION of p, obs(p), bad(j)); a map point "isBad" when no key-frame holds it, beObserved(T) means T holds it, and its
 * ATTRIBUTES are the ones replicated on its carriers, read from the lowest live one: position, normal, min / max distance,
 * ref_kf, point_desc.
 * enable_fuse(bounds, max_candidates): valid on an EMPTY store on which vo_kfstore_enable_point_upkeep has succeeded; bounds =
 * xMin, xMax, yMin, yMax of the undistorted image (xMax > xMin, yMax > yMin), the grid constants are 64 / (xMax - xMin) and
 * 48 / (yMax - yMin) in float (camera.cpp:47-48); max_candidates >= 1 bounds the candidates of one step and the matches of one
 * call, each of which reserves one node of the overlay; max_features above 4096 is VO_ERR_CAPACITY (a target's key-points are staged in 64 KB).  One device
 * block of 16 * index capacity + 28 * max_candidates + 244 * max_features bytes and a little.  Synchronises once.
 * fuse(T, list, threshold), the reference's loop in list order.  A candidate p is skipped unless: p >= 0; somebody holds it;
 * T does not; z >= 0 (float) in T's camera; isInImg(u, v) (keyframe.cpp:64-67, float); 0.8f * min <= dist <= 1.2f * max;
 * line . normal >= 0.5 * dist (double); level = predictScale (mappoint.cpp:198-212, as VO_TRACKER_* projections compute it).
 * Its window (keyframe.cpp:268-309) holds the features whose ROUNDED cell (frame.cpp:83-86; outside the 64 x 48 grid: none)
 * lies in the FLOOR-computed cell range of (u, v) +- radius, radius = threshold * scale_factors[level], and that have
 * |dx| < radius && |dy| < radius.  Of those with octave in [level - 1, level] and chi-square <= 7.815 (u_right >= 0; three
 * terms) or 5.991 (two), the strictly smallest Hamming distance between the candidate's point_desc and the feature's desc wins
 * in the order cell column, cell row, feature; a match needs distance <= 50.  Feature EMPTY (bit 0 clear): it gets p, bit 0
 * and p's attributes.  Feature carries org: obs(org) > obs(p) replaces p by org, otherwise org by p.
 * replace(A -> B): every holder j of A with observation i: j does not hold B -> feature (j, i) takes B's id and attributes;
 * else bit 0 of (j, i) is cleared.  Every other feature that carries A loses bit 0 too (a choice of this restatement: the
 * pointer model leaves a dangling bad pointer there).  When BOTH have an entry in the recent list B's found / visible grow by
 * A's; A's entry stays (the next cull removes it, branch 1).  Then compute_descriptors(B).
 * fuse_map_points(target, n, ids, threshold): one fuse call on its own.  target in [0, size), n in [0, 60 * max_features]
 * (else VO_ERR_CAPACITY), threshold > 0; one copy, one synchronisation at the end.  fuse_map_points_dev: ids in device memory,
 * ENQUEUED only (the index rebuilt first when stale, one memset, four launches).  target erased or without a pose: nothing
 * changes, VO_KFSTORE_CONNECTIONS_INVALID.  Afterwards the index is stale and the generation word has advanced.
 * search_in_neighbors(current): current in [0, size) validated, then ENQUEUED only.  The target list (:365-386): the first
 * 10 of current's ordered list, bad ones skipped, each followed by its own first 5 without the bad ones, the first neighbours
 * seen so far and current; only first neighbours are marked, so a key-frame can come several times and is fused several times
 * (at most 60 targets; the marks are per call, which differs from fuseKFId_ for key-frame id 0 only).  Then fuse(T, current's
 * ids in feature order as the call found them, 3) per target in list order; fuse(current, the targets' ids by first
 * occurrence over the target list, 3); compute_descriptors and vo_kfstore_refresh_points for current's live points; the
 * connection update of current.  The observation index is rebuilt once in front when stale and once before the closing
 * descriptors, whatever the number of targets; afterwards it is fresh.  current erased or without a pose: only the
 * connection update runs, VO_KFSTORE_CONNECTIONS_INVALID.
 * Capacity, three limits on the device: more than max_candidates candidates passing the gates in ONE step leave that step
 * undone; when the MATCHES of a call (each reserves one overlay node) exceed max_candidates, the step that meets the limit and
 * every later one are left undone; a replace between points of which one has more than VO_KFSTORE_FUSE_MAX_CARRIERS live
 * features is left undone.  Each raises the sticky VO_KFSTORE_FUSE_CAPACITY, which vo_kfstore_connections_status reads and
 * clears with 1 / 2 / 4 / 8; the record of an undone step keeps its candidates and matches.
 * fuse_result(record, targets, per_target): synchronises; any pointer may be NULL.  record [8] = number of steps, then the
 * totals of the six columns, 0; targets [61] = the target of every step (the closing step's is current); per_target [61][6] =
 * candidates that passed the gates, matches, adds, replaces that kept org, replaces that kept the candidate, features
 * cleared. */
#define VO_KFSTORE_FUSE_CAPACITY 16
#define VO_KFSTORE_FUSE_MAX_CARRIERS 1024
#define VO_KFSTORE_FUSE_MAX_STEPS 61
int vo_kfstore_enable_fuse(vo_kfstore *s, const float bounds[4] /*xMin xMax yMin yMax*/, int max_candidates);
int vo_kfstore_fuse_map_points(vo_kfstore *s, int target, int n, const int32_t *ids, float threshold);
int vo_kfstore_fuse_map_points_dev(vo_kfstore *s, int target, int n, const int32_t *dev_ids, float threshold);
int vo_kfstore_search_in_neighbors(vo_kfstore *s, int current);
int vo_kfstore_fuse_result(vo_kfstore *s, int32_t *record /*[8]*/, int32_t *targets /*[61]*/, int32_t *per_target /*[61][6]*/);
/* Loop Sim3 on the device: LoopClosing::computeSim3 (loopClosing.cpp:178-348) from the store, behind
 * vo_kfdb_query_loop[_dev] and the host's consistency groups.  Opt-in and additive: a store without it allocates and behaves
 * as before.  The definitions are section 4i's (HOLDS, OBSERVATION, bad(j)); a map point's position, descriptor, normal and
 * min / max distance are read at the feature through which the walk meets it.  A Sim3 is 13 doubles as vo_sim3_ransac_eval
 * writes them: R row-major, t, s.  The CONTRACT is the reference's sequential result.
 * enable_loop(max_candidates, max_loop_points, max_rand): valid on an EMPTY store on which vo_kfstore_enable_fuse has succeeded
 * (which implies connections, culling, mapping, local BA, point upkeep: poses, key-point xy / octave, bounds, normals);
 * max_candidates in [1, VO_KFSTORE_LOOP_MAX_CANDIDATES], max_loop_points >= 1, max_rand >= 3.  One device block of
 * 129 * max_candidates * max_features + 127 * max_features + 5 * index capacity + 21 * max_loop_points + 4 * max_rand bytes and
 * a little (alignment, one k_node_replay argument block per candidate); the table ransacMaxIters(N), N <= max_features, is
 * evaluated here with the host's C library (sim3Solver.cpp:86-93), so the device computes no log.  Synchronises once.
 * compute_sim3(current, cand[n_cand], fix_scale, rand_values[n_rand], rand_max, max_rounds): current and every candidate in
 * [0, size) (VO_ERR_INVALID), n_cand <= max_candidates and n_rand <= max_rand (VO_ERR_CAPACITY), rand_max >= 1 (the caller's
 * RAND_MAX); ONE copy up, the call enqueued, ONE synchronisation at the end.  compute_sim3_dev: cand and rand_values in device
 * memory, ENQUEUED only -- no host synchronisation, no device-to-host copy, no allocation; the key-frame numbers are checked
 * on the device (a number outside the store is a bad candidate).  current erased or without a pose: no walk, every result
 * zero, VO_KFSTORE_CONNECTIONS_INVALID.  Neither form touches an erase lock (vo_kfstore_set_erase_lock): the caller locks the
 * candidates and current beforehand and releases, by the final state, ACCEPTED: every candidate but the matched one (:331-339);
 * NO MATCH and REJECTED: every candidate and current (:290-296, :341-346); UNDECIDED: none yet.
 * 1. Front, all candidates at once: candidate i is discarded when bad(cand[i]) or erased (:210); else
 *    Matcher(0.75).searchByBoW(current, cand[i], checkRot = true) (matcher.cpp:561-677) over the store's FeatureVectors; fewer
 *    than 20 matches discard it (:218).
 * 2. Sim3Solver (sim3Solver.cpp:8-96) per live candidate, in feature order of current: a match at feature i is kept when
 *    feature i has bit 0 and an id >= 0 that current holds, and the matched feature's id >= 0 is held by the candidate (ids are
 *    validated where they enter and one call changes nothing, so only a store filled through the device forms can fail this;
 *    a candidate without a pose keeps no match and its solver stops at once); idx1 / idx2 are the OBSERVATIONS, which need not be i; pcam = Tcw * p in double;
 *    pixels = Camera::camera2pixel in double with the float intrinsics; maxError = (int)(9.210 * sigma * sigma);
 *    ransacMaxIters = max(1, min(ceil(log(0.01) / log(1 - pow((float)20 / N, 3))), 300)), 1 at N == 20.
 * 3. The walk (:234-288): while (candidates > 0 && !matchFlag) for i: iterate(5) on candidate i's solver, whose state persists
 *    (iterations_global_, inliers_best_, the >= against the best, the > 20 return, the N < 20 exit).  Every trip consumes
 *    three of rand_values in order, as randomInt does: int(((double)r / ((double)rand_max + 1.0)) * d) over the shrinking
 *    index list (:125-141).  A non-empty return is VERIFIED: inlierMappoints, searchBySim3(current, cand, ., Scm, 7.5)
 *    (matcher.cpp:679-865; z < 0 one way, z <= 0 the other), solveLoopSim3 (vo_sim3_solve's contract: Scm is written only when
 *    both problems ran); >= 20 inliers end the walk with Scw = Scm * Smw, otherwise it resumes behind candidate i.  The record
 *    reports rand_used.  A trip that would draw past n_rand leaves the call UNDECIDED for good and raises
 *    VO_KFSTORE_LOOP_RAND_SHORT; 3 * 300 * n_cand values always suffice.  A caller who shares rand() with others pre-draws,
 *    and afterwards re-seeds and discards rand_used values, so that its generator stands where the reference's would.
 * 4. Rounds.  A round is "walk to the next verification or to the end, then verify".  max_rounds rounds are enqueued
 *    unconditionally (five launches each); nothing synchronises in between, and a round whose predecessor finished returns
 *    at once.  Not finished after max_rounds: UNDECIDED, which is no error and raises nothing;
 *    compute_sim3_continue(max_rounds) enqueues more rounds on the state as left.  Results do not depend on the split.
 * 5. After a match (:298-347): the loop points are the ids of ALL of the matched key-frame's ordered list (section 4h) in its
 *    order, then the matched key-frame itself: bit 0 set, feature order, first occurrence.  The mark is per call, which differs
 *    from loopPointIdxOfKF_ only for a point marked by an earlier call on the same current.  More than max_loop_points:
 *    UNDECIDED for good, VO_KFSTORE_LOOP_CAPACITY.  Then searchByProjection(current, Scw, loopPoints, matchMapPoints, 10)
 *    (matcher.cpp:356-447) with its ordered claims and the :422 index quirk as vo_match_sim3_projection reproduces them;
 *    match_cnt >= 40 is ACCEPTED, else REJECTED.
 * loop_result: synchronises; any pointer may be NULL.  record [16] = state (0 UNDECIDED, 1 NO MATCH, 2 REJECTED, 3 ACCEPTED),
 * matched position in cand and key-frame (-1: none), rounds run, verifications, rand_used, the inlier count of the last
 * refinement, match_cnt, number of loop points, 0 ...; per_cand [max_candidates][8] = key-frame, discard reason (0 live, 1
 * bad, 2 below 20 BoW matches, 3 solver stopped), BoW matches, N, ransacMaxIters, iterations_global_, inliers_best_,
 * verifications; Scm / Scw [13] (Scw behind a match only); match_ids [features of current] = matchMapPoints_ as map-point ids,
 * -1 for null (behind a match; -1 otherwise); loop_point_ids [max_loop_points] = loopConnectKFMapPoints_ with
 * *n_loop_points entries (states 2 and 3).  Both lists stay on the device.
 * loop_solver_inputs(position): Sim3Solver's arrays of candidate `position` of the last call as its constructor left them
 * (*n = N; pcams1_ / pcams2_ [N][3], pixels1_ / pixels2_ [N][2], maxError1_ / maxError2_ [N], matchedIndexs_ [N]); synchronises;
 * any array may be NULL. */
#define VO_KFSTORE_LOOP_MAX_CANDIDATES 16
#define VO_KFSTORE_LOOP_RAND_SHORT 32
#define VO_KFSTORE_LOOP_CAPACITY 64
#define VO_KFSTORE_LOOP_UNDECIDED 0
#define VO_KFSTORE_LOOP_NO_MATCH 1
#define VO_KFSTORE_LOOP_REJECTED 2
#define VO_KFSTORE_LOOP_ACCEPTED 3
int vo_kfstore_enable_loop(vo_kfstore *s, int max_candidates, int max_loop_points, int max_rand);
int vo_kfstore_compute_sim3(vo_kfstore *s, int current, int n_cand, const int32_t *cand, int fix_scale, int n_rand,
                            const int32_t *rand_values, int32_t rand_max, int max_rounds);
int vo_kfstore_compute_sim3_dev(vo_kfstore *s, int current, int n_cand, const int32_t *dev_cand, int fix_scale, int n_rand,
                                const int32_t *dev_rand_values, int32_t rand_max, int max_rounds);
int vo_kfstore_compute_sim3_continue(vo_kfstore *s, int max_rounds);
int vo_kfstore_loop_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *per_cand /*[max_candidates][8]*/, double *Scm /*[13]*/,
                           double *Scw /*[13]*/, int32_t *match_ids /*[n of current]*/, int32_t *n_loop_points,
                           int32_t *loop_point_ids /*[max_loop_points]*/);
/* Sim3Solver::setRansacParameters(0.99, 20, 300) for n correspondences (sim3Solver.cpp:76-96), on the host: the entry of the
 * table enable_loop uploads.  1 for n <= 20. */
int vo_kfstore_loop_ransac_max_iters(int n);
int vo_kfstore_loop_solver_inputs(vo_kfstore *s, int position, int32_t *n, double *cam1_points, double *cam2_points, double *pixels1,
                                  double *pixels2, int32_t *max_err1, int32_t *max_err2, int32_t *matched_index);
/* The loop pose graph from the store: Optimizer::solvePoseGraphLoop (optimizer_ceres.cpp:1036-1305) with
 * the pose collection (:1062-1083) and the four edge families (:1094-1236) gathered on the device, and the write-back of
 * every key-frame pose (:1264-1278) and every map point (:1281-1301) done there; the solve in between is
 * vo_pose_graph_solve's, unchanged.  It takes LoopClosing::correctLoop's outputs as plain arrays, so a host correctLoop can
 * drive it.  Opt-in and additive: a store without it allocates and behaves as before, and every entry point of this block
 * returns VO_ERR_INVALID on it.  bad(j) and "erased" are section 4i's; pointer-keyed containers are walked in ascending
 * key-frame number.  A Sim3 is 8 doubles as vo_sim3_reanchor_points takes them: quaternion x y z w, translation, scale; every
 * Sim3 an entry point receives has its quaternion normalised when it is read.  All Sim3 arithmetic is csrc/sim3_compose.h's:
 * double, a fixed operation order, every operation rounded on its own (DESIGN.md section 4o writes the order down).
 * enable_pose_graph(max_edges, max_corrected, max_corrected_points): valid only on an EMPTY store on which
 * vo_kfstore_enable_local_ba has succeeded, else VO_ERR_INVALID; capacities below 1 are VO_ERR_INVALID.  Allocates, with K =
 * max_keyframes, N = max_features, Nn = min(K, 683) (the solver's 6 (nodes - 1) <= 4096), E / C / P the capacities and every
 * array rounded up to 16 bytes: the loop-edge rows and counts (36 K); node index, edge counts and the refresh list
 * (4 K N + 8 K + 4 C + 4); S_wr (64 Nn); a window's inputs (136 C + 4 E + 8 P + 4); the window -- the record (64), nodes
 * (68 Nn), edges (72 E); a solver's result (56 Nn): 4 K N + 44 K + 188 Nn + 76 E + 140 C + 8 P + 72 bytes as listed,
 * 2 813 160 at 500 key-frames of 1000 features with 8192 edges, 64 corrected key-frames and 8192 corrected points; and ONE
 * page-locked staging block of the largest of the window, the inputs and the result (host memory, 623 888 bytes there, before
 * the allocator's headroom).  Synchronises once.
 * add_loop_edge(a, b): KeyFrame::addLoopEdge both ways (loopClosing.cpp:484-485, keyframe.cpp:528-533): b joins a's loop
 * edges and a joins b's, and both get the erase lock of vo_kfstore_set_erase_lock(.., 1).  A repeat changes nothing.  At
 * most VO_KFSTORE_MAX_LOOP_EDGES per key-frame: VO_ERR_CAPACITY beyond, with nothing written.  a, b in [0, size), a != b, else
 * VO_ERR_INVALID.  Enqueues only.  get_loop_edges: synchronises; *n and edges [VO_KFSTORE_MAX_LOOP_EDGES] ascending.
 * pose_graph_window(curr, match, ...): corr_kf [n_corr] strictly ascending = the key set of both correctSim3 and
 * uncorrectSim3 (currConnectKFs_ with curr, loopClosing.cpp:367-398), S_corr / S_uncorr [n_corr][8]; lc_start [n_corr + 1]
 * (lc_start[0] == 0) and lc_kf = loopConnections as CSR over the same keys, each row strictly ascending; cp_id [n_cp] strictly
 * ascending with cp_ref = the points with loopCorrectByKF_ == curr and their correctReference_.  The host form validates all
 * of that, every number against [0, size) (ids: >= 0) and the counts against the capacities (VO_ERR_CAPACITY) before anything
 * is enqueued (VO_ERR_INVALID, nothing changes); ONE copy, four launches, synchronises once.  pose_graph_window_dev: the same
 * arrays in device memory with n_lc given; curr, match and the counts are validated, the arrays are copied device to device
 * and everything is ENQUEUED only -- no host synchronisation, no device-to-host copy, no allocation; what the host form
 * validates is checked on the device: a violation gives status EMPTY and the sticky VO_KFSTORE_CONNECTIONS_INVALID.  The
 * window is that of the reference called once:
 *  1 nodes: the key-frames that are not erased, ascending and compacted; node_kf[i] = the key-frame of node i.  More than Nn
 *    nodes or more than max_edges edges: status OVERFLOW, the record holds the TRUE counts, no array is valid, the sticky
 *    VO_KFSTORE_POSE_GRAPH_CAPACITY is raised.  curr or match erased, or any node without a pose: status EMPTY and the sticky
 *    VO_KFSTORE_CONNECTIONS_INVALID (vo_kfstore_connections_status reads and clears both).
 *  2 node Sim3 (:1062-1083): S_corr where the key-frame is in corr_kf, else (unit_quaternion(R), t, 1) from the pose column
 *    (Eigen's four branches); quats / trans / scales hold it with the quaternion normalised, and it is these values every
 *    later step reads.
 *  3 family A (:1094-1125): keys ascending, each row ascending; k -> j is emitted when W[k][j] >= 100 (quirk Q-B5: the curr /
 *    match exemption never acts) and both are nodes and j != k; the measurement is S[j] * S[k]^-1 on the node Sim3s; the pair
 *    joins `inserted`.
 *  4 per node key-frame k ascending, with Swi = (S_uncorr[k] if listed, else k's node Sim3)^-1 and the other end resolved
 *    the same way, measurement S[other] * Swi (:1128-1236): B the parent, when k has one and it is a node; C k's loop edges l
 *    ascending with l < curr (:1174) that are nodes; D the prefix of k's ordered list (section 4h) with weight >= 100
 *    (getCovisiblesByWeight, keyframe.cpp:341-356) in list order, skipping an entry w that is the parent, a child of k (a
 *    non-erased key-frame whose parent is k), a loop edge of k, bad(w), w >= k, or with (w, k) in `inserted`.
 *  5 edge_i / edge_j are node indices in exactly this order (the solver's sums follow it): per-row and per-key-frame counts, a
 *    scan, an emit at the offsets; no atomics decide an order.
 * pose_graph_window_result: synchronises (one copy into the staging block); record [16] = n_nodes, n_edges, the counts of
 * families A, B, C, D, status (VO_KFSTORE_BA_WINDOW_*), curr, match, fixed_node (match's node), and of the last apply
 * n_points_moved and n_unanchored (feature rows, not distinct points); four zeros.  Arrays filled to the counts when the status
 * is OK: node_kf, quats [n][4], trans [n][3], scales, edge_i, edge_j, q_meas [e][4], t_meas [e][3], s_meas (the caller sizes
 * them by Nn and max_edges).  Any pointer may be NULL.
 * pose_graph_apply(quats, trans): a solver's result for the LAST window, host arrays in node order; one copy, three launches,
 * one synchronisation at the end.  VO_ERR_INVALID when there is no window, the last one is empty or overflowed, or the store
 * has been changed since (the generation word of local_ba_apply; add_loop_edge advances it).  In the reference's order:
 *  a every node, the fixed one included, gets Tiw = SE3(normalised uq, t / s) as Tcw12 in the pose column, and
 *    Swr = Sim3(s, R(Tiw), t)^-1, with s the window's scale of the node.
 *  b every feature with bit 0 set of every non-erased key-frame: idm = cp_ref where its id is in cp_id, else its ref_kf as
 *    stored; its row becomes Swr[idm] * (Srw[idm] * p), Srw being the window's node Sim3 (step 2).  The row is the feature's own,
 *    so the carriers of a point with equal rows and equal ref_kf end with equal rows.  idm == -1 or not a node: the row keeps
 *    its bytes and counts in n_unanchored (the reference reads a default-constructed Sim3 there).
 *  c every live point is refreshed as by vo_kfstore_refresh_points (updateNormalAndDepth, :1299).
 *  d the observation index is marked stale and the generation word advances.
 * pose_graph(curr, match, ..., max_iterations, summary): the window, ONE device-to-host copy into the staging block,
 * vo_pose_graph_solve(n_nodes, ..., fixed_node, ..., fix_scale = 1, max_iterations, summary) on those bytes, the apply.
 * Whatever the solver refuses is returned and NOTHING is written back (the rule of the C++ shim's solvePoseGraphLoop);
 * VO_ERR_CAPACITY for an overflowed window, VO_ERR_INVALID for an empty one.  summary may be NULL.  Running the solver on the
 * window's device arrays in place is not covered. */
#define VO_KFSTORE_MAX_LOOP_EDGES 8
#define VO_KFSTORE_POSE_GRAPH_CAPACITY 128
int vo_kfstore_enable_pose_graph(vo_kfstore *s, int max_edges, int max_corrected, int max_corrected_points);
int vo_kfstore_add_loop_edge(vo_kfstore *s, int a, int b);
int vo_kfstore_get_loop_edges(vo_kfstore *s, int keyframe, int32_t *n, int32_t *edges /*[VO_KFSTORE_MAX_LOOP_EDGES]*/);
int vo_kfstore_pose_graph_window(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *corr_kf, const double *S_corr,
                                 const double *S_uncorr, const int32_t *lc_start, const int32_t *lc_kf, int n_cp, const int32_t *cp_id,
                                 const int32_t *cp_ref);
int vo_kfstore_pose_graph_window_dev(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr,
                                     const double *dev_S_uncorr, const int32_t *dev_lc_start, int n_lc, const int32_t *dev_lc_kf, int n_cp,
                                     const int32_t *dev_cp_id, const int32_t *dev_cp_ref);
int vo_kfstore_pose_graph_window_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *node_kf, double *quats, double *trans,
                                        double *scales, int32_t *edge_i, int32_t *edge_j, double *q_meas, double *t_meas, double *s_meas);
int vo_kfstore_pose_graph_apply(vo_kfstore *s, const double *quats, const double *trans);
int vo_kfstore_pose_graph(vo_kfstore *s, int curr, int match, int n_corr, const int32_t *corr_kf, const double *S_corr,
                          const double *S_uncorr, const int32_t *lc_start, const int32_t *lc_kf, int n_cp, const int32_t *cp_id,
                          const int32_t *cp_ref, int max_iterations, vo_lm_summary *summary);
/* The loop fusion on the device: LoopClosing::searchAndFuse (loopClosing.cpp:496-516) with
 * Matcher::fuseByPose (matcher.cpp:1135-1238) and MapPoint::replaceMapPoint (mappoint.cpp:214-253) on the store, the step of
 * correctLoop between its pose propagation and the pose graph.  Opt-in and additive: a store without it allocates and behaves
 * as before.  The definitions, a map point's "isBad", beObserved and ATTRIBUTES, and replace(A -> B) with its carrier limit are
 * the fusion block's above; corr_kf and S_corr are the arrays vo_kfstore_pose_graph_window[_dev] takes, so one upload serves both.
 * enable_loop_fuse(max_corrected, max_loop_points): valid on an EMPTY store on which vo_kfstore_enable_fuse has succeeded,
 * capacities >= 1, else VO_ERR_INVALID.  One device block of 16 + up16(4 (C + 1)) + 32 C + 64 C + up16(4 C) + up16(4 P) bytes
 * (C = max_corrected, P = max_loop_points): the call's head, per pass its first match and its record, and the host form's
 * arrays.  It works on the fusion layer's overlay and match list: enable_fuse's max_candidates bounds the candidates that pass
 * the gates in ONE pass and the matches of one CALL.  Synchronises once.
 * search_and_fuse(n_corr, corr_kf, S_corr, n_points, ids, threshold): n_corr passes, T = corr_kf[0], corr_kf[1], ... (strictly
 * ascending: correctPose is walked in ascending key-frame number), each fuseByPose(T, S_corr[T], ids, replace, threshold) and
 * then replace[i] -> replaceMapPoint(ids[i]) in list order.  S_corr: 8 doubles per key-frame, quaternion x y z w (normalised
 * when read), translation, scale.  ids: loopConnectKFMapPoints_ in list order, distinct (a negative entry is skipped).
 *  1. Tcw = SE3(R(q), t), t NOT divided by the scale (matcher.cpp:1144), Ow = -(R^T t); doubles, each operation rounded.
 *  2. Candidate i is skipped unless: id >= 0; somebody holds it (a loop point replaced in an earlier pass is bad); T does not;
 *     z >= 0 (float); isInImg(u, v); 0.8f * min <= dist <= 1.2f * max; line . normal >= 0.5 * dist (double); level =
 *     predictScale.  These are the fusion block's gates with the Sim3's pose in place of T's pose column.
 *  3. The window is the fusion block's with radius = threshold * scale_factors[level]; of its features with octave in
 *     [level - 1, level] -- there is NO chi-square gate and no u_right -- the strictly smallest Hamming distance between the
 *     candidate's point_desc and the feature's desc wins in the order cell column, cell row, feature; a match needs <= 50.
 *  4. Feature EMPTY (bit 0 clear): it takes the candidate's id, bit 0 and attributes at once; a later candidate of the pass
 *     that hits it finds that loop point there.  Feature carries org: replace[i] = org, nothing is written yet.
 *  5. After the list, in list order: replace(replace[i] -> ids[i]), always org -> loop point.  An org a former replace of the
 *     pass has emptied is NOT skipped: no carrier moves, the counters are added once more when both are in the recent list,
 *     compute_descriptors(ids[i]) runs.  A == B by id does nothing.
 *  6. Afterwards the index is stale and the generation word has advanced.  Connections are NOT updated (correctLoop calls
 *     vo_kfstore_update_connections itself, :469).  A T outside [0, size), erased or without a pose column gives a pass that
 *     changes nothing and raises VO_KFSTORE_CONNECTIONS_INVALID.
 *  7. Capacity, three limits on the device, each raising VO_KFSTORE_FUSE_CAPACITY: more than max_candidates candidates passing in
 *     one pass leave that pass undone; matches of the call beyond max_candidates leave that pass and every later one undone;
 *     a replace between points of which one has more than VO_KFSTORE_FUSE_MAX_CARRIERS live features is left undone.
 * The host form validates: n_corr > max_corrected or n_points > max_loop_points is VO_ERR_CAPACITY; corr_kf not strictly
 * ascending, threshold <= 0, a negative count or a NULL array with a positive count VO_ERR_INVALID, nothing changed; ONE copy
 * up, the call enqueued, one synchronisation.  search_and_fuse_dev: the same arrays in device memory, read in place; counts
 * and NULLs validated as above, everything else on the device; ENQUEUED only: the index rebuilt first when stale, three
 * memsets, 1 + 2 n_corr launches (1 when n_points is 0), no host synchronisation, no copy, no allocation.
 * search_and_fuse_loop: the loop points are the list the last vo_kfstore_compute_sim3 left on the device, read in place; needs
 * vo_kfstore_enable_loop (else VO_ERR_INVALID); ENQUEUED only, the same launches.  A last call whose state is not
 * VO_KFSTORE_LOOP_ACCEPTED is decided on the device: nothing changes, the record has 0 passes, VO_KFSTORE_CONNECTIONS_INVALID.
 * loop_fuse_result(record, per_pass): synchronises; either pointer may be NULL.  record [8] = passes run, then the totals of
 * the six columns, 0; per_pass [max_corrected][6] = candidates that passed the gates, matches, adds, replaces recorded,
 * replaces that moved at least one carrier, features cleared (rows beyond the passes are 0). */
int vo_kfstore_enable_loop_fuse(vo_kfstore *s, int max_corrected, int max_loop_points);
int vo_kfstore_search_and_fuse(vo_kfstore *s, int n_corr, const int32_t *corr_kf, const double *S_corr /*[n_corr][8]*/, int n_points,
                               const int32_t *ids, float threshold);
int vo_kfstore_search_and_fuse_dev(vo_kfstore *s, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr, int n_points,
                                   const int32_t *dev_ids, float threshold);
int vo_kfstore_search_and_fuse_loop(vo_kfstore *s, int n_corr, const int32_t *dev_corr_kf, const double *dev_S_corr, float threshold);
int vo_kfstore_loop_fuse_result(vo_kfstore *s, int32_t *record /*[8]*/, int32_t *per_pass /*[max_corrected][6]*/);
/* The loop correction on the device: the two steps of LoopClosing::correctLoop that PRODUCE the arrays
 * vo_kfstore_search_and_fuse_loop and vo_kfstore_pose_graph_window_dev take -- the propagation of the loop Sim3 over the current
 * key-frame's neighbours with the correction of their map points (loopClosing.cpp:364-437) and the loop connections (:461-479).
 * Opt-in and additive: a store without it allocates and behaves as before.  A Sim3 is 8 doubles (quaternion x y z w,
 * translation, scale); all Sim3 arithmetic is csrc/sim3_compose.h's, every operation rounded on its own; pointer-keyed
 * containers are walked in ascending key-frame number; "holds", bit 0, bad(j), "erased" are the culling block's definitions.
 * enable_loop_correct(max_corrected, max_corrected_points, max_loop_connections): valid on an EMPTY store on which
 * vo_kfstore_enable_pose_graph has succeeded, capacities >= 1, else VO_ERR_INVALID.  One device block of
 *   64 + 16 + 64 + up16(4 K) + up16(4 C) + 64 C + up16(4 B) + up16(4 P) + up16(C K)
 *   + 2 up16(4 C) + 128 C + 2 up16(4 P) + up16(4 (C + 1)) + up16(4 E)   bytes
 * (K = max_keyframes, C, P, E the three capacities, B = the observation index's capacity / 256): the record, the one-entry list
 * of step 1, the Sim3 as received, position-in-corr_kf per key-frame, the list position per corrected key-frame, S_corr^-1, a count per workgroup of the index grid, the entry of every corrected point, a loop-connection row
 * per list position; then the result, contiguous: list, corr_kf, S_corr, S_uncorr, cp_id, cp_ref, lc_start, lc_kf.  It also
 * grows the connection layer's scratch (connections.hip: 16 n + 4 n K + 4 n bytes for a list of n entries, grow-only) to
 * n = max_corrected when it is smaller: a second allocation at most, here and not in a call.  Synchronises once.
 * Every propagate_loop and loop_connections call advances the generation word, also one that the device then refuses: the
 * host cannot know, and a window taken before the call is conservatively no longer applicable.
 * propagate_loop(curr, Scw[8]):
 *  1. update(curr) as vo_kfstore_update_connections does it; the index is rebuilt first when stale.
 *  2. currConnect = curr's ordered list as step 1 left it, then curr -- EVERY entry: isBad is not tested (:367).  It is kept in
 *     this order for loop_connections; corr_kf is the same set strictly ascending.  More than max_corrected entries: status
 *     OVERFLOW and the sticky VO_KFSTORE_CORRECT_LOOP_CAPACITY.  curr or a listed key-frame erased or without a pose column, or a
 *     scale of Scw that is not > 0 (step 6 divides by it):
 *     status EMPTY and the sticky VO_KFSTORE_CONNECTIONS_INVALID.  In either case nothing beyond step 1 is written.
 *  3. S_uncorr[k] = s3_from_pose(T_k); S_corr[curr] = s3_load(Scw); for every other k, Swc = s3_inv(s3_from_pose(T_curr)),
 *     Sic = s3_mul(S_uncorr[k], Swc), S_corr[k] = s3_mul(Sic, Scw): the reference's SE3 algebra as Sim3 algebra at scale 1.
 *  4. corr_kf ascending, features ascending, bit 0 set: a point is corrected ONCE, through the lowest-numbered corrected
 *     key-frame k that holds it, at its first carrying feature there, whose row is p:
 *     p' = s3_act(s3_inv(S_corr[k]), s3_act(S_uncorr[k], p)), written to every live feature that carries the id, in EVERY
 *     key-frame.  cp_ref of the point is k; cp_id is strictly ascending.  More than max_corrected_points: status OVERFLOW, the
 *     sticky VO_KFSTORE_CORRECT_LOOP_CAPACITY, nothing beyond step 1 written.
 *  5. updateNormalAndDepth of the point at once (:426), on the poses the reference's loop has at that moment: a holder, or the
 *     reference key-frame, that is a corrected key-frame at a position of corr_kf BELOW k's has its corrected pose (step 6);
 *     one at k's position or above, and one outside corr_kf, its stored pose.  Since k is the LOWEST corrected key-frame that
 *     holds the point, and the reference key-frame is a holder, no holder lies below k: every pose is the stored one, although
 *     step 6 overwrites it in the same call.  Everything else is vo_kfstore_refresh_points' contract and operation order.  A
 *     point is refreshed once.
 *  6. The pose column of corr_kf[j] becomes SE3(s3_matrix(q), t / s) of S_corr[j] (q normalised as step 3 left it, each
 *     division rounded on its own).
 *  7. update(k) for k in corr_kf ascending, as one update_connections list.
 *  8. The generation word advances; the observation index stays valid (no id and no flag changes).
 * The host form copies Scw up, enqueues, synchronises once; curr outside [0, size) or Scw NULL is VO_ERR_INVALID.
 * propagate_loop_dev(curr, dev_Scw): Scw in device memory, read in place; ENQUEUED only: the index rebuilt when stale, one memset,
 * 12 launches, no host synchronisation, no device-to-host copy, no allocation.  propagate_loop_sim3(): curr and Scw (13
 * doubles R, t, s -> s3_from_pose(R, t) with the scale appended) where the last vo_kfstore_compute_sim3 left them, read in
 * place; needs vo_kfstore_enable_loop (else VO_ERR_INVALID); ENQUEUED only.  A state other than VO_KFSTORE_LOOP_ACCEPTED is
 * decided on the device: nothing changes, status EMPTY, VO_KFSTORE_CONNECTIONS_INVALID.
 * loop_connections(): after the caller's search_and_fuse.  For kf in currConnect in LIST order: old = the members of kf's ordered
 * list as this step finds it (after the updates of the earlier entries of this loop); update(kf); new = { j : W[kf][j] != 0 } as
 * the step leaves it (the whole weight map; an update that finds no connection leaves the old row);
 * loopConnections[kf] = new \ old \ currConnect, fixed at its own step.  Output: CSR over corr_kf ascending (lc_start [n_corr + 1],
 * lc_kf, every row strictly ascending).  More than max_loop_connections: connections status OVERFLOW, the sticky
 * VO_KFSTORE_CORRECT_LOOP_CAPACITY, no array valid.  The connection state afterwards is that of
 * vo_kfstore_update_connections(currConnect in list order).  Without a successful propagate_loop before it (none since enable, or
 * the last one refused): nothing changes, connections status EMPTY, VO_KFSTORE_CONNECTIONS_INVALID.  ENQUEUED only: the index
 * rebuilt when stale, four launches; the generation word advances.
 * loop_correct_result(record, list, corr_kf, S_corr, S_uncorr, cp_id, cp_ref, lc_start, lc_kf): synchronises; any pointer may be
 * NULL.  record [16] = n_corr, n_cp, n_lc, curr, status of the last propagate (VO_KFSTORE_BA_WINDOW_OK / _EMPTY / _OVERFLOW), the
 * feature rows step 4 wrote, status of the last loop_connections, 0 ...  The arrays are cut to the counts (nothing is copied
 * for a status that is not OK); list [n_corr] is currConnect in list order.
 * loop_correct_arrays(...): the DEVICE addresses of corr_kf, S_corr, S_uncorr, cp_id, cp_ref, lc_start and lc_kf (any pointer may
 * be NULL); no synchronisation.  They stay where they are for the store's life; their contents are those of the last calls. */
#define VO_KFSTORE_CORRECT_LOOP_CAPACITY 256
int vo_kfstore_enable_loop_correct(vo_kfstore *s, int max_corrected, int max_corrected_points, int max_loop_connections);
int vo_kfstore_propagate_loop(vo_kfstore *s, int curr, const double *Scw /*[8]*/);
int vo_kfstore_propagate_loop_dev(vo_kfstore *s, int curr, const double *dev_Scw);
int vo_kfstore_propagate_loop_sim3(vo_kfstore *s);
int vo_kfstore_loop_connections(vo_kfstore *s);
int vo_kfstore_loop_correct_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *list, int32_t *corr_kf, double *S_corr, double *S_uncorr,
                                   int32_t *cp_id, int32_t *cp_ref, int32_t *lc_start, int32_t *lc_kf);
int vo_kfstore_loop_correct_arrays(vo_kfstore *s, const int32_t **dev_corr_kf, const double **dev_S_corr, const double **dev_S_uncorr,
                                   const int32_t **dev_cp_id, const int32_t **dev_cp_ref, const int32_t **dev_lc_start,
                                   const int32_t **dev_lc_kf);
/* The merge of the loop matches on the device: the loop of LoopClosing::correctLoop that gives the current
 * key-frame the loop's map points (loopClosing.cpp:439-455), between propagate_loop and search_and_fuse; and the composed
 * vo_kfstore_correct_loop.  Opt-in and additive: a store without it allocates and behaves as before.  "Holds", "observation",
 * isBad ("nobody holds it"), a point's attributes (those of its lowest live carrier), replace(A -> B) with its carrier limit and
 * compute_descriptors are the fusion block's definitions.
 * enable_loop_merge(): valid on an EMPTY store on which vo_kfstore_enable_loop_fuse has succeeded, else VO_ERR_INVALID.  One
 * device block of
 *   16 + 64 + 6 up16(4 NK)   bytes, NK = max_features:
 * the call's head, the record (16 ints), per feature of the current key-frame the step's plan (the branch taken, ALONE / ORDERED,
 * the ordered steps' features, the overlay node of an add: two words), and the host form's match_ids.  Synchronises once.  The
 * calls work on the fusion layer's overlay slots (reset at the start of a call) with the nodes of this block, one per feature, so
 * that an add never meets max_candidates; the match list and the records of the last fuse / search_and_fuse call survive.
 * merge_loop_matches(curr, n, match_ids): for i ascending over [0, min(n, features of curr)) with B = match_ids[i] >= 0, each step
 * on the state the steps before it left:
 *  - NO-OP: feature i of curr has bit 0 and carries A >= 0 with A == B: nothing happens, no descriptor is recomputed
 *    (mappoint.cpp:216).
 *  - DEAD B: nobody holds B when the step comes (an earlier step of the call replaced it away, or the caller handed in a dead id).
 *    The reference would copy a dead object's attributes; the store has none: the step is skipped and counted.
 *  - REPLACE: feature i has bit 0 and carries A >= 0, A != B: replace(A -> B) as the fusion block defines it -- an observation of
 *    A whose key-frame does not hold B takes B's id and attributes, every other carrier of A loses bit 0, the recent-list counters
 *    are added when both are listed, compute_descriptors(B).  Always org -> loop point: no observation count is compared.  More
 *    than VO_KFSTORE_FUSE_MAX_CARRIERS live features on either side: left undone, the sticky VO_KFSTORE_FUSE_CAPACITY.
 *  - ADD: feature i has bit 0 clear (or a negative id): it takes B's id, bit 0 and B's attributes, then compute_descriptors(B).
 *    Whether curr holds B at another feature already is NOT tested (the reference does not): the id then stands in two features
 *    of curr, and curr's observation is the lowest-numbered of them (the pointer model keeps the one registered first).  A B that
 *    then has more than VO_KFSTORE_FUSE_MAX_CARRIERS live features keeps its descriptor, the sticky VO_KFSTORE_UPKEEP_CAPACITY.
 *  There is no updateNormalAndDepth in either branch.  Afterwards the observation index is stale and the generation word has
 *  advanced; connections are NOT updated (the reference updates them at :469: vo_kfstore_loop_connections).
 * Decided on the device: curr outside [0, size) or erased, or (the _loop form) a compute_sim3 state other than
 * VO_KFSTORE_LOOP_ACCEPTED: nothing changes, the record shows 0 steps, VO_KFSTORE_CONNECTIONS_INVALID.
 * The host form validates before anything is enqueued: n > max_features VO_ERR_CAPACITY; n < 0, or NULL with n > 0,
 * VO_ERR_INVALID (so do the _dev form's); then ONE copy up, the enqueue, ONE synchronisation.  merge_loop_matches_dev: the list in
 * device memory, read in place; ENQUEUED only: the index rebuilt when stale, two memsets, four launches, no host synchronisation,
 * no device-to-host copy, no allocation.  merge_loop_matches_loop(): curr, matchMapPoints_ and its length where the last
 * vo_kfstore_compute_sim3 left them, read in place; needs vo_kfstore_enable_loop (else VO_ERR_INVALID); ENQUEUED only.
 * loop_merge_result(record, per_feature): synchronises; either may be NULL.  record [16] = steps (entries >= 0), adds, no-ops,
 * replaces recorded (carried out or left undone), replaces that moved at least one carrier, features cleared, dead Bs, replaces
 * left undone for the carrier limit, steps that ran on the ordered path (those that share an id with another step of the call),
 * curr, 0 ...; per_feature [max_features] = the branch at feature i: 0 none, 1 add, 2 no-op, 3 replace, 4 dead, 5 undone.
 * correct_loop(threshold, max_iterations, summary, record): correctLoop from :364 to :485 on the state the last compute_sim3
 * left; needs enable_loop, enable_loop_correct and enable_loop_merge (else VO_ERR_INVALID).  A fixed sequence:
 *  1. propagate_loop_sim3; 2. merge_loop_matches_loop; 3. ONE synchronising read (the propagation's record, the merge's,
 *  compute_sim3's state, the sticky word -- read, not cleared); 4. search_and_fuse_loop(n_corr, the layer's corr_kf and S_corr,
 *  threshold) (the reference passes 4); 5. loop_connections; 6. ONE synchronising read (n_lc, the connections status, the sticky
 *  word, the fusion's record); 7. pose_graph_window_dev on the layer's device arrays with curr and match of compute_sim3's record,
 *  then vo_kfstore_pose_graph's tail: the window copied down, vo_pose_graph_solve with fix_scale as compute_sim3 was called, the
 *  apply; 8. add_loop_edge(curr, match).
 * Returns VO_ERR_INVALID when the last compute_sim3 was not ACCEPTED or a step reports EMPTY; VO_ERR_CAPACITY when a step
 * overflowed or VO_KFSTORE_FUSE_CAPACITY stands in the sticky word at step 3 or 6 (a bit an earlier call left counts: read and
 * clear the word first); whatever the solver refuses as it is, with nothing written back by step 7 or 8.  The store is then as
 * the steps before the stop specify.  record [16] (may be NULL) = curr, match, n_corr, n_cp, n_lc, the merge's adds and replaces,
 * the fusion's totals of adds and replaces, the window's n_nodes and n_edges, the apply's n_points_moved (one more small read,
 * made only when record is given), the step at which the call stopped (0 = finished), 0 ... */
int vo_kfstore_enable_loop_merge(vo_kfstore *s);
int vo_kfstore_merge_loop_matches(vo_kfstore *s, int curr, int n, const int32_t *match_ids);
int vo_kfstore_merge_loop_matches_dev(vo_kfstore *s, int curr, int n, const int32_t *dev_match_ids);
int vo_kfstore_merge_loop_matches_loop(vo_kfstore *s);
int vo_kfstore_loop_merge_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *per_feature /*[max_features]*/);
int vo_kfstore_correct_loop(vo_kfstore *s, float threshold, int max_iterations, vo_lm_summary *summary, int32_t *record /*[16], may be NULL*/);
/* Loop detection on the device: LoopClosing::detectLoop (loopClosing.cpp:52-175) with the consistency
 * groups, the erase locks of the loop thread (setNotEraseLoopDetectingKF / setEraseLoopDetectingKF, keyframe.cpp:541-557) and ONE
 * iteration of LoopClosing::run (:17-37) as a composed call.  Opt-in and additive: a store without it allocates and behaves as
 * before.  The database is the vo_kfdb whose insertion numbers are the store's.
 * enable_detect_loop(D = max_detect_candidates, G = max_groups): valid on an EMPTY store on which vo_kfstore_enable_loop and
 * vo_kfstore_enable_pose_graph have succeeded (the layer reads the loop edges for the lock rule and hands over to compute_sim3),
 * with 1 <= D <= G <= VO_KFSTORE_DETECT_MAX_GROUPS; anything else VO_ERR_INVALID.  One device block of
 *   64 + 64 + 96 + 2 up16(4 D) + up16(8 G) + 2 up16(4 K) + 16 G W + up16(8 D W) + up16(D G)   bytes,
 *   K = max_keyframes, W = ceil(K / 64), up16(x) = x rounded up to 16:
 * the words the calls hand on, the record, the lock record, candidates and the enough list, the groups' counters (two halves),
 * the query's excl and conn lists, the groups as bitsets over key-frames (two halves), the candidates' bitsets and the
 * consistency bytes.  Synchronises once.
 * detect_loop(db, current, last_loop_keyframe): detectLoop for key-frame `current`, which the caller has inserted into db already
 * (the reference adds a key-frame to the map before the loop thread sees it, map.cpp:224-226); the query's BoW vector is db's own
 * row of `current`.  ENQUEUED ONLY: six launches on the store's stream (plus the four that rebuild db's index after an
 * insertion), db's stream ordered around them by events; no host synchronisation, no device-to-host copy, no allocation.  Checked
 * on the host before anything is enqueued, each VO_ERR_INVALID: the layer enabled, db given, current in [0, size),
 * last_loop_keyframe >= 0, db and the store holding the same number of key-frames.  On the device, in the reference's order:
 *  1. the erase lock of `current` is set (:59).
 *  2. current < last_loop_keyframe + 10 (:62): GATED.  The groups are not touched; the lock is released by the rule below.
 *  3. conn = `current`'s ordered list as the connection state holds it, without the key-frames flagged bad (:72-76), in list
 *     order; excl = every j with W[current][j] != 0, and `current` (map.cpp:212-215).
 *  4. min_score as vo_kfdb_query_loop computes it from conn (1.0f for an empty list).
 *  5. db's neighbour rows are refreshed from the store: EVERY key-frame in [0, size) gets the first VO_KFSTORE_MAX_NEIGHBORS of its
 *     ordered list (its graph row), so that getBestCovisibleKFs(10) of map.cpp:284 is the store's.  This OVERWRITES what
 *     vo_kfdb_set_neighbors / _batch put there.  (A GATED call returns before it, as the reference does.)
 *  6. one loop query, vo_kfdb_query_loop_dev's kernel unchanged, max_out = D.
 *  7. no candidate (:87-93): the groups are cleared, NO_CANDIDATES, the lock is released.
 *  8. DEVIATION: a true candidate count above D, or more than G groups in step 9: OVERFLOW, the sticky VO_KFSTORE_DETECT_CAPACITY
 *     (vo_kfstore_connections_status), the groups are cleared, the lock is released.  The reference's vectors grow instead.
 *  9. the consistency groups (:95-165) exactly as written: the group of candidate c is { j : W[c][j] != 0 } and c itself, bad and
 *     erased members included (getConnectKFs filters nothing); candidates in query order, previous groups in stored order; a
 *     candidate is CONSISTENT with a previous group when the two share a key-frame; the first candidate consistent with previous
 *     group j pushes (its group, count of j + 1) and flags j, later ones push nothing for j (:142-147); a candidate joins the
 *     enough list at most once, when such a count reaches 3, flagged or not (:149-153); a candidate consistent with no previous
 *     group pushes (its group, 0) (:158-162); the new list replaces the old one (:165).
 * 10. the enough list empty: NOT_CONSISTENT, the lock is released (:167-171).  Else DETECTED: the lock stays, and the enough list
 *     stays on the device for compute_sim3_detected.
 * The lock RELEASE of this block is setEraseLoopDetectingKF: the lock comes off only when the key-frame has no loop edge
 * (vo_kfstore_add_loop_edge); nothing is erased; a released key-frame whose `pending` word is set (vo_kfstore_cull_state) is
 * reported, and the caller calls vo_kfstore_erase_keyframe (vo_kfstore_set_erase_lock's contract).  A `current` that is erased:
 * nothing runs, no lock is touched, outcome NONE, the sticky VO_KFSTORE_CONNECTIONS_INVALID.
 * detect_loop_result(record, candidates, enough): synchronises; each may be NULL.  record [16] = outcome (below), current, n_excl,
 * n_conn, min_score as its float bits (0 when the call did not get that far), the TRUE candidate count, groups before, groups
 * after, n_enough, the lock of `current` afterwards, its pending word, 0 ...; candidates [D] and enough [D]: the first min(count, D)
 * / n_enough entries are written.
 * detect_loop_groups(n, counts, members): synchronises; prevConsistentGroups_ as the layer holds it: *n groups, counts [G], and
 * members [G][size] bytes (1: the key-frame is in the group); entries beyond *n are not written.
 * compute_sim3_detected(fix_scale, n_rand, rand_values, rand_max, max_rounds) / _dev: vo_kfstore_compute_sim3 for `current` and the
 * enough list of the last detect_loop, read in place (the _dev form takes rand_values in device memory and is ENQUEUED only; the
 * host form copies them up and synchronises once at its end).  It sets the erase lock of every enough candidate first (:208),
 * enqueues the front for max_candidates of the loop layer and leaves every array a result reads byte-identical to
 * vo_kfstore_compute_sim3 called with the same list.  Unless the last outcome is DETECTED it walks nothing, leaves the loop layer's
 * state NO MATCH with zero candidates and raises VO_KFSTORE_CONNECTIONS_INVALID; more enough candidates than max_candidates:
 * the same with VO_KFSTORE_LOOP_CAPACITY instead.  No detect_loop enqueued on this store yet: VO_ERR_INVALID.
 * release_loop_locks(): ENQUEUED only, one launch.  The releases computeSim3 ends with (:290-296, :331-346), by the state of the
 * last compute_sim3*: ACCEPTED every candidate but the matched one; NO MATCH and REJECTED every candidate and `current`;
 * UNDECIDED none.  Each follows the release rule above.  loop_locks_result(n_released, n_pending, pending): synchronises; the
 * number of key-frames the call released the lock of, and those of them whose pending word is set (at most
 * VO_KFSTORE_LOOP_MAX_CANDIDATES + 1).
 * set_ / get_last_loop_keyframe: lastLoopKFId_ of the composed step (0 on a new store, as in the reference's constructor).
 * loop_closing_step(db, current, fix_scale, n_rand, rand_values, rand_max, max_rounds, threshold, max_iterations, summary,
 * record): one iteration of LoopClosing::run for key-frame `current`; needs enable_detect_loop and what vo_kfstore_correct_loop
 * needs.  A fixed sequence of this header's entry points, no kernel of its own:
 *  1. detect_loop(db, current, the last-loop word); 2. compute_sim3_detected in its host form, without its synchronisation and
 *  without the sticky bit for an outcome other than DETECTED (how almost every key-frame ends);
 *  3. ONE synchronising read: the detect record and compute_sim3's state; a key-frame that ends GATED, NO_CANDIDATES,
 *  NOT_CONSISTENT or OVERFLOW costs exactly this one synchronisation; 4. while UNDECIDED: compute_sim3_continue(max_rounds) and one
 *  read of the state each, until it is decided or a pass adds no round (the rand() values have run out: returned as UNDECIDED, no
 *  lock released); 5. release_loop_locks; 6. on ACCEPTED vo_kfstore_correct_loop(threshold, max_iterations, summary), and on its
 *  success the last-loop word becomes `current` (:491).
 * record [16] (may be NULL) = the detect outcome, compute_sim3's state (-1: not reached), correct_loop's return code (1: not
 * reached), the step at which it stopped, n_enough, the matched key-frame or -1, continue passes, the last-loop word afterwards,
 * 0 ...  Returns the first failing entry point's code (OVERFLOW: VO_ERR_CAPACITY; an erased `current`: VO_ERR_INVALID), else
 * VO_OK; the arguments are checked before anything is enqueued (more rand() values than max_rand: VO_ERR_CAPACITY). */
#define VO_KFSTORE_DETECT_CAPACITY 512
#define VO_KFSTORE_DETECT_MAX_GROUPS 1024
#define VO_KFSTORE_DETECT_NONE 0
#define VO_KFSTORE_DETECT_GATED 1
#define VO_KFSTORE_DETECT_NO_CANDIDATES 2
#define VO_KFSTORE_DETECT_NOT_CONSISTENT 3
#define VO_KFSTORE_DETECT_DETECTED 4
#define VO_KFSTORE_DETECT_OVERFLOW 5
int vo_kfstore_enable_detect_loop(vo_kfstore *s, int max_detect_candidates, int max_groups);
int vo_kfstore_detect_loop(vo_kfstore *s, vo_kfdb *db, int current, int last_loop_keyframe);
int vo_kfstore_detect_loop_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *candidates /*[D]*/, int32_t *enough /*[D]*/);
int vo_kfstore_detect_loop_groups(vo_kfstore *s, int32_t *n, int32_t *counts /*[G]*/, uint8_t *members /*[G][size]*/);
int vo_kfstore_compute_sim3_detected(vo_kfstore *s, int fix_scale, int n_rand, const int32_t *rand_values, int32_t rand_max, int max_rounds);
int vo_kfstore_compute_sim3_detected_dev(vo_kfstore *s, int fix_scale, int n_rand, const int32_t *dev_rand_values, int32_t rand_max,
                                         int max_rounds);
int vo_kfstore_release_loop_locks(vo_kfstore *s);
int vo_kfstore_loop_locks_result(vo_kfstore *s, int32_t *n_released, int32_t *n_pending, int32_t *pending /*[17]*/);
int vo_kfstore_set_last_loop_keyframe(vo_kfstore *s, int keyframe);
int vo_kfstore_get_last_loop_keyframe(vo_kfstore *s, int32_t *keyframe);
int vo_kfstore_loop_closing_step(vo_kfstore *s, vo_kfdb *db, int current, int fix_scale, int n_rand, const int32_t *rand_values,
                                 int32_t rand_max, int max_rounds, float threshold, int max_iterations, vo_lm_summary *summary,
                                 int32_t *record /*[16], may be NULL*/);
/* Key-frame creation on the device: a tracked frame written into the store as a key-frame --
 * VisualOdometry::createNewKeyFrame (visualOdometry.cpp:463-517) with cullingTempMapPoints' slot rule (:844-853), and the first
 * key-frame of initVisualOdometry (:170-198) -- for a caller who keeps no host copy of ids or flags: the link between "frame
 * tracked" and vo_kfstore_process_new_keyframe.  Opt-in and additive: a store without it allocates and behaves as before.  The
 * definitions are section 4i's (j HOLDS p, j's OBSERVATION of p, obs(p), bad(j)).
 * enable_keyframe_create: valid on an EMPTY store on which vo_kfstore_enable_local_ba has succeeded (poses, xy, octave / depth /
 * u_right, the id counter, normals, ref_kf and the observation index); anything else VO_ERR_INVALID.  One device block of
 *   8 P + up16(8 NK) + 64 + 16 + 16 + 5 up16(4 NK) + up16(8 NK) + up16(96 + 7 up16(4 NK) + 32 NK)   bytes, NK = max_features,
 *   P = the power of two >= NK, up16(x) = x rounded up to 16:
 * the sort keys, the created rows, the record (16 ints), need_stats' counts, the effective count, the step's scratch (slot, first observation, new
 * id, word, node per feature; weight) and the host forms' staging (Tcw12, seven columns, the descriptors).  Synchronises once.
 * create_keyframe_dev(vocab, n, dev_Tcw12, dev_x, dev_y, dev_octave, dev_angle, dev_depth, dev_u_right, dev_desc, dev_slot_ids,
 * th_depth, initial, index): validated on the host: 0 <= n <= max_features (itself <= 16384, the FeatureVector kernel's sort:
 * vo_kfstore_enable_mapping refuses a wider store) and a free key-frame (else VO_ERR_CAPACITY), vocab and
 * the arrays present, dev_desc on a 16-byte boundary (else VO_ERR_INVALID).  *index = the store's size before the call.
 * Everything else is ENQUEUED on the store's stream -- the index rebuilt first when stale, then four launches (walk, fill,
 * k_bow_transform, k_featvec): no host synchronisation, no device-to-host copy, no allocation; the arrays must stay untouched
 * until the stream has passed the call.  dev_slot_ids[i] = frame_curr_->mappoints_[i] as a global map-point id, negative =
 * null, as the slots stand when the reference calls createNewKeyFrame (before cullingOutliersOfFrame).  In the reference's order:
 *  1 temp cull (:844-853): a slot whose id is negative, or whose id no non-erased key-frame holds (getObsCnt() < 1 decided by
 *    holders, section 4l's rule), is NULL -- which makes `!mp || mp->getObsCnt() < 1` (:493) one condition.  The key-frame
 *    being created is not among the holders.
 *  2 depth walk (:469-513, initial == 0): the pairs (d, i) with d > 0 (float compare: NaN, -0 and -1 are out) ascending by d,
 *    then i (sort on pair<float, int>, a total order).  c_j = 1 where pair j's slot is null, C_j its inclusive prefix sum, J the
 *    first j with d_j > th_depth && C_j > 100, or the last pair.  The check follows the creation: the pair at which the count
 *    reaches 101 is created when it is far, and a far TRACKED pair behind 101 creations ends the walk too.  Exactly the pairs
 *    j <= J with c_j = 1 get a new point, id = counter + C_j - 1 (factory_id_++ in walk order); the counter advances by C_J.
 *  3 initial == 1 (:179-198): every feature with !(d < 0), in feature order, gets a point; ids ascend with the feature index.
 *    d == 0 and NaN are created (quirk Q-V1).  dev_slot_ids is ignored and may be NULL.
 *  4 a created point (camera.cpp:82-94, mappoint.cpp:36-50, 52-64, 66-116, 118-179 with one observation):
 *    x = ((u - cx) * d) / fx and likewise y in float, every operation rounded, widened to double; p_w = R^T (p_c - t) on Tcw12
 *    in double (q = p_c + (-t), p_w[i] = (R[0][i] q[0] + R[1][i] q[1]) + R[2][i] q[2]; Sophus' quaternion rounding is not
 *    reproduced).  flags = 3, ids = the new id, ref_kf = the new key-frame, point_desc = the feature's descriptor, normal and
 *    min / max distance what vo_kfstore_refresh_points computes for one holder (a later refresh changes no byte).
 *  5 a tracked slot (not null after 1, with or without depth): flags = 3, ids = the slot's id; points, point_desc, normal,
 *    min / max distance and ref_kf are copied from the id's first observation: the lowest non-erased key-frame that holds it,
 *    at that key-frame's observation.  vo_kfstore_process_new_keyframe refreshes them afterwards.
 *  6 a null slot that gets no point: flags 0, id -1, ref_kf -1, zero columns.
 *  7 angle, desc, octave / depth / u_right, xy and the pose with its pose-set word are copied; the FeatureVector is built by
 *    k_bow_transform (levelsup 3) and k_featvec; bad = 0.  The observation index is stale afterwards and the generation word has
 *    advanced.  Graph row and connections are vo_kfstore_process_new_keyframe's.
 * create_keyframe: the same from host arrays; octave within the store's levels is validated too (VO_ERR_INVALID); one staging
 * copy, one synchronisation at the end.  On an error nothing changes.
 * create_keyframe_from_frames(vocab, frames, slot, n, dev_Tcw12, dev_slot_ids, th_depth, initial, index): the feature columns
 * are those of `slot` of a vo_frames handle (the one vo_tracker_frames returns: an extracted frame never leaves the device);
 * slot and n <= the frames' capacity are validated too.  n is the caller's (VO_TRACKER_KEYPOINT_COUNTS, vo_frames_download): if
 * it differs from the slot's count on the device the key-frame gets n = 0 features in its head, the n rows the getters span
 * are written as null slots without a feature (zeros; id, ref_kf, depth, u_right -1), the record's status is 1 and the sticky
 * VO_KFSTORE_CONNECTIONS_INVALID is raised.  The store's stream waits, by an event, for what the
 * stream that last wrote the frames (vo_frames_build_dev, vo_frames_upload) holds at the call; ENQUEUED like the device form.
 * keyframe_result(record, created_feature, created_id): synchronises; any pointer may be NULL.  record [16] = key-frame, n,
 * depth pairs, pairs walked (J + 1), n_created, n_tracked, first id, next id, whether the walk ended early, status (0, or 1:
 * the frames form's n was not the slot's), six zeros (initial: the "pairs" are the features with !(d < 0)).  created_feature / created_id [n_created] in walk order.
 * keyframe_need_stats_dev(ref_kf, min_obs, n, dev_depth, dev_slot_ids, th_depth, dev_out): the three counts of needNewKeyFrame
 * (:406-428), nothing of its decision.  ENQUEUED: one launch behind the index rebuild.  out[0] =
 * keyframe_trackRef_->trackedMapPoints(min_obs) (keyframe.cpp:210-226): features of ref_kf with bit 0 whose obs(p) >= min_obs;
 * out[1] = map_cnt, out[2] = total_cnt over the frame's features with 0 < d < th_depth (a slot counts when some non-erased
 * key-frame holds its id); out[3] = 0.  ref_kf erased or outside the store: zeros and the sticky
 * VO_KFSTORE_CONNECTIONS_INVALID.  keyframe_need_stats: host arrays in (n <= max_features), out [4] on the host; one copy up, one
 * down, one synchronisation. */
int vo_kfstore_enable_keyframe_create(vo_kfstore *s);
int vo_kfstore_create_keyframe_dev(vo_kfstore *s, const vo_vocab *vocab, int n, const double *dev_Tcw12, const float *dev_x,
                                   const float *dev_y, const int32_t *dev_octave, const float *dev_angle, const float *dev_depth,
                                   const float *dev_u_right, const uint8_t *dev_desc, const int32_t *dev_slot_ids, float th_depth,
                                   int initial, int32_t *index);
int vo_kfstore_create_keyframe(vo_kfstore *s, const vo_vocab *vocab, int n, const double *Tcw12, const float *x, const float *y,
                               const int32_t *octave, const float *angle, const float *depth, const float *u_right, const uint8_t *desc,
                               const int32_t *slot_ids, float th_depth, int initial, int32_t *index);
int vo_kfstore_create_keyframe_from_frames(vo_kfstore *s, const vo_vocab *vocab, vo_frames *frames, int slot, int n,
                                           const double *dev_Tcw12, const int32_t *dev_slot_ids, float th_depth, int initial,
                                           int32_t *index);
/* The feature side of a key-frame as the store holds it (read-only, beside vo_kfstore_get_points; needs vo_kfstore_enable_mapping):
 * angle, desc [n][32], octave, depth, u_right, xy [n][2] (n as inserted) and the FeatureVector -- n_nodes, node [n_nodes], start
 * [n_nodes + 1], feat [start[n_nodes]], in arrays of n (start: n + 1) entries.  Any pointer may be NULL.  Synchronises. */
int vo_kfstore_get_features(vo_kfstore *s, int keyframe, float *angle, uint8_t *desc, int32_t *octave, float *depth, float *u_right,
                            float *xy, int32_t *n_nodes, int32_t *node, int32_t *start, int32_t *feat);
int vo_kfstore_keyframe_result(vo_kfstore *s, int32_t *record /*[16]*/, int32_t *created_feature, int32_t *created_id);
int vo_kfstore_keyframe_need_stats_dev(vo_kfstore *s, int ref_kf, int min_obs, int n, const float *dev_depth,
                                       const int32_t *dev_slot_ids, float th_depth, int32_t *dev_out /*[4]*/);
int vo_kfstore_keyframe_need_stats(vo_kfstore *s, int ref_kf, int min_obs, int n, const float *depth, const int32_t *slot_ids,
                                   float th_depth, int32_t *out /*[4]*/);
/* vo_tracker_relocalize with the candidates read from a store: dev_cand [batch][cand_stride] key-frame numbers in walk
 * order and dev_n_cand [batch] in device memory -- the output layout of vo_kfdb_query_reloc_dev.  The first
 * min(n_cand[f], max_reloc_candidates) of a frame are walked.  Frame construction, computeBow, the frames' FeatureVectors
 * (k_featvec), the candidates' records gathered from the store, their global ids mapped to dense ids per frame, the
 * common-node walk (k_bow_walk), k_node_replay and the rest of the route as vo_tracker_relocalize has it: all enqueued, no
 * host synchronisation, no device-to-host copy, and no allocation after the first call (which sizes the route's buffers
 * from the tracker's capacities).  The store's max_features must not exceed max_reloc_features (VO_ERR_CAPACITY at the
 * call).  Results are bit-identical to vo_tracker_set_reloc_candidates + vo_tracker_relocalize on the same key-frames;
 * VO_TRACKER_RELOC_POINT_IDS reports the store's global ids.  Conditions only the device sees are sticky and reported by
 * vo_tracker_results: a frame with more candidates than max_reloc_candidates -> VO_ERR_CAPACITY (its first
 * max_reloc_candidates are walked and every output is valid); a candidate outside [0, store size) -> VO_ERR_INVALID (that
 * candidate is walked as a bad key-frame, outcome 0; every other output is valid).  The candidates handed to
 * vo_tracker_set_reloc_candidates are gone after these calls (set them again before vo_tracker_relocalize).
 * vo_tracker_relocalize_db: the same with Map::detectRelocalizationCandidates in front -- vo_bow_vector_dev on the
 * transform's words and weights, the database query with max_out = max_reloc_candidates, on the tracker's stream;
 * dev_stale_score [size] or NULL as in vo_kfdb_query_reloc_dev.  db and store must hold the same number of key-frames
 * (VO_ERR_INVALID) and the database's max_batch must cover the batch (VO_ERR_CAPACITY), checked before anything is enqueued. */
int vo_tracker_relocalize_store(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_n_cand,
                                const int32_t *dev_cand, int cand_stride, const uint8_t *images, const void *depth,
                                int depth_kind, const vo_tracker_params *params);
int vo_tracker_relocalize_store_dev(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_n_cand,
                                    const int32_t *dev_cand, int cand_stride, const uint8_t *dev_images, int image_pitch,
                                    size_t image_frame_stride, const void *dev_depth, int depth_kind,
                                    size_t depth_frame_stride, int depth_pitch, const vo_tracker_params *params);
int vo_tracker_relocalize_db(vo_tracker *t, vo_kfdb *db, const vo_kfstore *store, const vo_vocab *vocab,
                             const float *dev_stale_score, const uint8_t *images, const void *depth, int depth_kind,
                             const vo_tracker_params *params);
int vo_tracker_relocalize_db_dev(vo_tracker *t, vo_kfdb *db, const vo_kfstore *store, const vo_vocab *vocab,
                                 const float *dev_stale_score, const uint8_t *dev_images, int image_pitch,
                                 size_t image_frame_stride, const void *dev_depth, int depth_kind, size_t depth_frame_stride,
                                 int depth_pitch, const vo_tracker_params *params);
/* vo_tracker_set_ref_keyframe + vo_tracker_track_ref_keyframe with the reference key-frames read from a store: the
 * reference key-frame of frame f is key-frame dev_ref_kf[f] (device memory, [batch]) and its start pose dev_Tcw12
 * [batch][12] (device memory; frame_last_->Tcw_, rotation row-major + translation).  Frame construction, computeBow, the
 * frames' FeatureVectors (k_featvec), the key-frames' points and flags gathered from the store into the last-frame arrays
 * together with the start pose and its se3 logarithm (k_ref_kf_gather), the common-node walk (k_bow_walk, one pair per
 * frame, Matcher(params->ref_ratio), 0.7 when not positive), k_node_replay and the tail of vo_tracker_track_ref_keyframe:
 * all enqueued, no host synchronisation, no device-to-host copy, and no allocation after the first store route of the
 * tracker that needs larger walk buffers than the routes used before it (they are sized for max_last features per
 * key-frame here, for max_reloc_features on the relocalisation routes, and only ever grow).  The tracker needs no relocalisation route
 * configured.  The store's max_features must not exceed max_last (VO_ERR_CAPACITY at the call, nothing enqueued).  A
 * key-frame flagged bad in the store is searched like any other: searchByBoW(KeyFrame*, Frame*) tests the map points
 * (matcher.cpp:476), never the key-frame.  Bit 1 of the store's flags (observe_cnt_ > 0) is read here, as after
 * vo_tracker_set_ref_keyframe.  Results are bit-identical to vo_tracker_set_ref_keyframe + vo_tracker_track_ref_keyframe
 * on the same key-frames.  Like vo_tracker_set_ref_keyframe the call REPLACES the last-frame state, and the reference
 * key-frame handed to vo_tracker_set_ref_keyframe earlier is gone after it.  A key-frame number outside [0, store size)
 * is searched as a key-frame without features: that frame gets 0 matches and VO_TRACK_FEW_MATCHES, every other frame's
 * outputs are valid, and vo_tracker_results reports the condition as sticky VO_ERR_INVALID (the word of the store routes
 * of relocalisation).  dev_ref_kf and dev_Tcw12 must stay untouched until the stream has passed the call. */
int vo_tracker_track_ref_keyframe_store(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab,
                                        const int32_t *dev_ref_kf, const double *dev_Tcw12, const uint8_t *images,
                                        const void *depth, int depth_kind, const vo_tracker_params *params,
                                        int first_stage_only);
int vo_tracker_track_ref_keyframe_store_dev(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab,
                                            const int32_t *dev_ref_kf, const double *dev_Tcw12, const uint8_t *dev_images,
                                            int image_pitch, size_t image_frame_stride, const void *dev_depth, int depth_kind,
                                            size_t depth_frame_stride, int depth_pitch, const vo_tracker_params *params,
                                            int first_stage_only);
/* VisualOdometry::updateLocalKeyFrames + updateLocalMapPoints (visualOdometry.cpp:595-724) for every frame of the batch,
 * on the device, from the key-frame store: the step between a store route and vo_tracker_track_local_map.  Valid after
 * vo_tracker_relocalize_store / _db (and their _dev forms) and after vo_tracker_track_ref_keyframe_store[_dev] with
 * first_stage_only = 1; after any other route: VO_ERR_INVALID, nothing enqueued.  The slot ids of frame f are what
 * VO_TRACKER_RELOC_POINT_IDS holds (after a relocalisation), or store.ids[ref_kf[f]][assigned_last[i]] of every slot i
 * that still holds a point after the culling (reference-key-frame route; there `store` must be the store the route read,
 * after a relocalisation any store in the same id space serves).  Four steps, all enqueued on the tracker's stream, ordered
 * against the store's stream by events like the store routes, no host synchronisation, no allocation after the first
 * call (a later call with a store of more max_keyframes grows the vote buffer):
 *  1 votes (:598-614): every non-null slot gives one vote to every key-frame that holds its id (the observation index); an
 *    id in two slots votes twice.  A slot whose id no key-frame holds is `mp->isBad()`: it is nulled (:612) --
 *    VO_TRACKER_FEATURE_HAS_POINT cleared, its VO_TRACKER_RELOC_POINT_IDS entry -1.
 *  2 voters (:625-639) in ascending key-frame number (the ordering rule of vo_kfstore_set_graph), key-frames flagged bad
 *    skipped; the best key-frame is the first with the strictly largest count.
 *  3 expansion (:641-690) over the ORIGINAL voters in order, stopping once the list holds more than 80: per voter the
 *    first non-bad unmarked neighbour, the first non-bad unmarked child, the parent if unmarked and not bad.
 *  4 points (:700-724): the list's key-frames in list order, each one's features in index order with bit 0 set, first
 *    occurrence of an id wins; written straight into the local-map arrays (position, normal, min / max distance, the
 *    store's point_desc, flags = the feature's bits 0 and 1, the ids of vo_tracker_set_local_map_ids).  The local map's n
 *    becomes max_local; entries beyond a frame's count get flags 0 and id -1.  link: -1 after a relocalisation (the id
 *    skip acts there); on the reference-key-frame route the lowest feature index of the frame's reference key-frame that
 *    holds the same id with bit 0 set, or -1 -- vo_tracker_track_local_map then runs unchanged on either route.
 * Deviations, all stated: (a) a frame without voters gets an EMPTY local map and best key-frame -1, where the reference
 * returns early (:616) and keeps the previous frame's list, which the independent frames of a batch do not have; so does a
 * frame with VO_TRACK_RELOC_FAILED, of which nothing else is touched.  (b) The expansion walks the original voters only:
 * the reference caches the end iterator before its pushes (:641) and stays defined only while reserve(3 * voters) holds.
 * (c) The list holds VO_TRACKER_LOCAL_MAX_KEYFRAMES = 84 entries: 80 voters + 3 is the most an expansion reaches, and a
 * frame with 81 .. 84 voters keeps them all (no expansion, :643); a frame with MORE voters keeps the first 84 in key-frame
 * order, VO_TRACKER_LOCAL_N_KEYFRAMES reports its true count and vo_tracker_results the sticky VO_ERR_CAPACITY (the best
 * key-frame is still taken over all voters).  (d) A frame with more distinct points than max_local keeps the first
 * max_local in order, VO_TRACKER_LOCAL_N_POINTS reports the true count: sticky VO_ERR_CAPACITY as well; every other
 * frame's outputs are valid.  The addVisible / addFound counters: vo_tracker_point_stats (below).
 * The motion route: the call is also valid after vo_tracker_track_first[_dev] when the last-frame list it searched carries ids
 * (after vo_tracker_end_frame or vo_tracker_set_last_frame_ids); without ids on the list, and after vo_tracker_track[_dev]
 * (both stages in one call), it stays VO_ERR_INVALID.  The slot id of slot i < n is last_ids[VO_TRACKER_ASSIGNED_LAST[i]] where
 * VO_TRACKER_FEATURE_HAS_POINT[i] is set after cullingOutliersBeforeLocalMap and the assignment is >= 0, else -1: a temporary
 * point of updateLastFrame has no id, casts no vote and is not nulled.  One more launch in front gathers the ids
 * (VO_TRACKER_FIRST_SLOT_IDS: these ids after step 1's nulling, which clears VO_TRACKER_FEATURE_HAS_POINT as above), one behind
 * writes link[j] = the lowest last-list index with local point j's id and bit 0 set, or -1 -- step 3 of vo_tracker_begin_frame,
 * the same code, over EVERY entry of the list (all n of a list the host set, up to max_last, also where max_last > max_features)
 * -- and the link is in force, so that searchLocalMapPoints' skip (:753) acts in vo_tracker_track_local_map as on
 * a local map the host set.  Deviations (a) - (d) apply unchanged; `store` is any store in the id space of the last ids. */
#define VO_TRACKER_LOCAL_MAX_KEYFRAMES 84
int vo_tracker_build_local_map(vo_tracker *t, vo_kfstore *store);
/* With vo_tracker_set_timing on, a store route records HIP events around its four new stages: 0 k_featvec, 1 the gather
 * from the store, 2 the id compaction, 3 k_bow_walk.  Synchronises and returns the milliseconds of the LAST such call
 * (VO_ERR_INVALID when none has run with timing on).  tools/reloc_db_bench.py. */
#define VO_TRACKER_RELOC_STAGES 4
int vo_tracker_get_reloc_timing(vo_tracker *t, double *ms /*VO_TRACKER_RELOC_STAGES*/);
/* Waits for the batch and copies out (any pointer may be NULL): poses as se3 [batch][6] and as Tcw
 * [batch][12]; n_tracked = inliers of the second solve whose map point has observations (inliers_num_,
 * :289-300); n_inliers = the second solve's return value; the two searches' match counts; status bits.
 * Reports sticky stage errors (dropped key-points, exhausted candidate pools) as VO_ERR_CAPACITY, and the two sticky
 * conditions of vo_tracker_relocalize_store / _db and vo_tracker_track_ref_keyframe_store (above); the outputs are copied
 * out before it reports. */
int vo_tracker_results(vo_tracker *t, double *poses6, double *Tcw12, int32_t *n_tracked, int32_t *n_inliers,
                       int32_t *n_matches_last, int32_t *n_matches_local, int32_t *status);
/* intermediate state of the last batch (tests, shims): [batch][max_features] / [batch][max_local] arrays */
enum {
  VO_TRACKER_ASSIGNED_LAST = 0,      /* int32: last-frame point index per feature after search 1, or -1 */
  VO_TRACKER_ASSIGNED_LOCAL = 1,     /* int32: local point index per feature claimed by search 2, or -1 */
  VO_TRACKER_POSE_FIRST = 2,         /* double [batch][6]: pose after the first solve */
  VO_TRACKER_INLIERS_FIRST = 3,      /* int32 [batch]: return value of the first solve */
  VO_TRACKER_OBSERVED_INLIERS_FIRST = 4, /* int32 [batch]: cullingOutliersBeforeLocalMap's return value */
  VO_TRACKER_FEATURE_HAS_POINT = 5,  /* uint8: frame->mappoints_[i] != nullptr at the end */
  VO_TRACKER_FEATURE_POINTS = 6,     /* double [..][3]: that map point's position */
  VO_TRACKER_LOCAL_FLAGS = 7, VO_TRACKER_LOCAL_U = 8, VO_TRACKER_LOCAL_V = 9, VO_TRACKER_LOCAL_UR = 10,
  VO_TRACKER_LOCAL_LEVEL = 11, VO_TRACKER_LOCAL_VIEWCOS = 12, /* Frame::isInFrame's outputs per local point */
  VO_TRACKER_KEYPOINT_COUNTS = 13,   /* int32 [batch] */
  VO_TRACKER_FEATURE_OUTLIER = 14,   /* uint8: frame->outliers_[i] after the second solve (valid after the local-map stage) */
  /* after vo_tracker_relocalize ([batch][max_reloc_candidates] = the configured capacity as the row length) */
  VO_TRACKER_RELOC_WINNER = 15,      /* int32 [batch]: index of the candidate that relocalised the frame, -1 on failure */
  VO_TRACKER_RELOC_POINT_IDS = 16,   /* int32 [batch][max_features]: id of frame->mappoints_[i] at the end, -1 = null */
  VO_TRACKER_RELOC_BOW_MATCHES = 17, /* int32 [batch][max_reloc_candidates]: searchByBoW's return value (0: bad / absent) */
  VO_TRACKER_RELOC_PNP_INLIERS = 18, /* int32 [..][..]: poseEstimateByPnP's return value (0: not run) */
  VO_TRACKER_RELOC_OUTCOME = 19,     /* int32 [..][..]: 0 bad, 1 < 15 BoW matches, 2 < 10 PnP inliers, 3 < 10 solve inliers,
                                        4 below 50 at the end, 5 success, 6 not reached */
  VO_TRACKER_RELOC_PNP_MASK = 20,    /* uint8 [batch][max_reloc_candidates][max_features] (debug): per frame feature 0 = no
                                        PnP correspondence, 1 = correspondence, RANSAC outlier, 2 = RANSAC inlier */
  /* after vo_tracker_relocalize_store / _db */
  VO_TRACKER_RELOC_CANDIDATES = 21,  /* int32 [batch][max_reloc_candidates]: the key-frame numbers walked, -1 beyond them */
  VO_TRACKER_RELOC_N_CANDIDATES = 22, /* int32 [batch]: the frame's true candidate count (may exceed max_reloc_candidates) */
  /* after vo_tracker_build_local_map */
  VO_TRACKER_LOCAL_KEYFRAMES = 23,   /* int32 [batch][VO_TRACKER_LOCAL_MAX_KEYFRAMES]: localKeyframes_ in list order, -1 beyond */
  VO_TRACKER_LOCAL_N_KEYFRAMES = 24, /* int32 [batch]: the list's length (the true voter count where it exceeds 84) */
  VO_TRACKER_LOCAL_N_POINTS = 25,    /* int32 [batch]: distinct local points of the frame (may exceed max_local) */
  VO_TRACKER_LOCAL_REF_KF = 26,      /* int32 [batch]: keyframe_best (:692-696), -1 without voters */
  /* the local map as it stands ([batch][max_local]; set by vo_tracker_set_local_map / _ids or built) */
  VO_TRACKER_LOCAL_POINT_IDS = 27,   /* int32: map-point id per local point, -1 beyond a built frame's count */
  VO_TRACKER_LOCAL_POINTS = 28, VO_TRACKER_LOCAL_NORMALS = 29, /* double [..][3] */
  VO_TRACKER_LOCAL_MIN_DISTANCE = 30, VO_TRACKER_LOCAL_MAX_DISTANCE = 31, /* float */
  VO_TRACKER_LOCAL_DESC = 32,        /* uint8 [..][32] */
  VO_TRACKER_LOCAL_MAP_FLAGS = 33,   /* uint8: the flags as set / built (VO_TRACKER_LOCAL_FLAGS: after isInFrame) */
  VO_TRACKER_LOCAL_LINK = 34,        /* int32 */
  VO_TRACKER_POSE_START = 35,        /* double [batch][6]: the se3 the route's first solve started from: log of the Tcw given
                                        (vo_tracker_set_last_frame, vo_tracker_set_ref_keyframe, and computed on the device
                                        by vo_tracker_track_ref_keyframe_store and vo_tracker_begin_frame) */
  /* the hand-over (vo_tracker_end_frame / vo_tracker_begin_frame below) */
  VO_TRACKER_SLOT_IDS = 36,          /* int32 [batch][max_features]: id of frame->mappoints_[i] after cullingTempMapPoints, -1 = null */
  VO_TRACKER_SLOT_DESC = 37,         /* uint8 [batch][max_features][32]: that map point's descriptor (zeros: null) */
  VO_TRACKER_FRAME_POSE = 38,        /* double [batch][12]: R, t of exp(pose) of the frame handed over */
  VO_TRACKER_VELOCITY = 39,          /* double [batch][12]: Tcl_ */
  VO_TRACKER_MOTION_STATE = 40,      /* int32 [batch]: motionModel_ */
  VO_TRACKER_TEMP_COUNT = 41,        /* int32 [batch]: updateLastFrame's temporary points (C_J) */
  /* the last-frame list as it stands ([batch][max_last]; set by vo_tracker_set_last_frame / _ids or handed over) */
  VO_TRACKER_LAST_POINTS = 42,       /* double [..][3] */
  VO_TRACKER_LAST_FLAGS = 43,        /* uint8 */
  VO_TRACKER_LAST_OCTAVE = 44,       /* int32 */
  VO_TRACKER_LAST_ANGLE = 45,        /* float */
  VO_TRACKER_LAST_DESC = 46,         /* uint8 [..][32] */
  VO_TRACKER_LAST_IDS = 47,          /* int32: map-point id per entry, -1 = none */
  VO_TRACKER_LAST_N = 48,            /* int32 [1]: the list's n */
  VO_TRACKER_TCW_START = 49,         /* double [batch][12]: the pose the last-frame points are projected with (Tcw12 of
                                        vo_tracker_set_last_frame / _ref_keyframe, or VELOCITY * last pose of vo_tracker_begin_frame) */
  /* the motion route from the key-frame store (vo_tracker_point_stats etc. below) */
  VO_TRACKER_FIRST_SLOT_IDS = 50,    /* int32 [batch][max_features]: id of frame->mappoints_[i] when the local-map stage starts, as
                                        vo_tracker_build_local_map gathered it from the last ids, after its nulling; -1 = null or temporary */
  VO_TRACKER_STAT_IDS = 51,          /* int32 [batch][max_features + max_local]: vo_tracker_point_stats' rows */
  VO_TRACKER_STAT_VISIBLE = 52,      /* int32, same shape */
  VO_TRACKER_STAT_FOUND = 53,        /* int32, same shape */
  VO_TRACKER_REF_TCR = 54,           /* double [batch][12]: TcrDB_ of the remembered reference key-frame */
  VO_TRACKER_REF_KF = 55,            /* int32 [batch]: that key-frame's number, -1: none */
  VO_TRACKER_FEATURE_OBSERVED = 56   /* uint8 [batch][max_features]: the per-slot observed mark (bit 1 of the flags of the entry the
                                        slot took its point from); read by vo_tracker_end_frame[_store]'s cullingTempMapPoints */
};
int vo_tracker_get(vo_tracker *t, int what, void *dst, size_t dst_bytes);
/* frame_last_ = frame_curr_ on the device: what VisualOdometry::run does between two frames
 * (visualOdometry.cpp:80-128) and the preamble of trackWithMotion (:233-236), for every frame of the batch, so that
 * vo_tracker_track*_dev follows vo_tracker_track*_dev with nothing but launches in between.  The calls produce, on the device,
 * the arrays vo_tracker_set_last_frame fills from the host; no existing array moves.  Their own state is ONE device block,
 * allocated by the first call of any of the five functions below:
 *   slot ids 4 BF, slot descriptors 32 BF, slot flags BF, last ids 4 BL, three poses 3 x 96 B (+ B validity bytes), two counts
 *   2 x 4 B, and 8 BP sort keys only where P > 4096    (B = batch, F = max_features, L = max_last, P = the power of two >= F;
 *   every array rounded up to 4 KiB).
 * vo_tracker_set_last_frame_ids(n, ids [batch][n]): the map-point id of every entry of the last-frame list, negative = none; the
 * last-frame counterpart of vo_tracker_set_local_map_ids.  n must be the list's n (else VO_ERR_INVALID); the ids belong to the
 * list they were set for (vo_tracker_set_last_frame, vo_tracker_set_ref_keyframe and the store form of trackRefKeyFrame forget
 * them).  One copy, one synchronisation.
 * vo_tracker_set_last_pose(Tcw12 [batch][12], valid [batch]): frame_last_->Tcw_ and poseExist_ per frame -- the seed of the
 * motion model, and how a caller applies the local-BA refresh of :547-549.  One copy, one synchronisation.
 * vo_tracker_end_frame(p): :80-128.  Valid after vo_tracker_track[_dev] and vo_tracker_track_first[_dev], with or without
 * vo_tracker_track_local_map behind it; after any other route, or before any, VO_ERR_INVALID; max_features > max_last
 * VO_ERR_CAPACITY; in both cases nothing is enqueued and nothing changes.  ENQUEUED on the tracker's stream, one workgroup per
 * frame: no host synchronisation, no device-to-host copy, no allocation after the first call.  Per frame, slot i < n:
 *  1 the slot's source: VO_TRACKER_ASSIGNED_LOCAL[i] >= 0 -> that local point (id: vo_tracker_set_local_map_ids' or -1; the local
 *    point's descriptor); else VO_TRACKER_ASSIGNED_LAST[i] >= 0 and the slot non-null -> that last-frame entry (id: the last id or
 *    -1; that entry's descriptor); else null.  observed = the tracker's per-slot mark (bit 1 of the source's flags); outlier =
 *    VO_TRACKER_FEATURE_OUTLIER, 0 when the local-map stage did not run (the first stage has nulled its outliers already).
 *  2 cullingTempMapPoints (:844-853): a non-null slot without the observed mark becomes null, its outlier flag 0.  SLOT_IDS,
 *    SLOT_DESC are the slots as they stand now -- as the reference has them at createNewKeyFrame, BEFORE cullingOutliersOfFrame:
 *    what vo_kfstore_create_keyframe*'s dev_slot_ids asks for.  The tracker's own per-slot arrays are not written.
 *  3 ok = status == 0 && n_tracked >= min_tracked (<= 0: 30, :310; the 50 of :307 is the caller's through min_tracked).
 *  4 FRAME_POSE = R, t of exp(pose) (the arithmetic of vo_se3_exp).  ok and the last pose valid: VELOCITY = FRAME_POSE *
 *    last pose^-1 (csrc/handover_geom.h's operation order), MOTION_STATE = 1; else VELOCITY = identity, MOTION_STATE = 0
 *    (:94-103, :115-118).  The last pose becomes FRAME_POSE, valid when ok.
 *  5 cullingOutliersOfFrame (:888-895) and :128: the last-frame list becomes the frame.  Entry i is slot i, LAST_N =
 *    max_features; flags bit 0 = non-null and no outlier, bit 1 = non-null and observed; point, id, descriptor the slot's (zeros,
 *    -1 for a null slot); octave and angle the frame feature's.  Entries from n on: flags 0, id -1, zeros.  The list carries ids
 *    from here on.  A lost frame's list is handed over too (:128); the caller picks the next route from MOTION_STATE.
 * vo_tracker_begin_frame(p, dev_is_keyframe [batch] or NULL): valid after vo_tracker_end_frame with no track call and no
 * last-frame setter in between (the depth and feature columns are read from the frame store's slots, not copied), else
 * VO_ERR_INVALID.  ENQUEUED, one workgroup per frame:
 *  1 updateLastFrame's temporary points (:555-592), skipped for a frame with dev_is_keyframe[f] != 0 (:552): the pairs (d, i)
 *    with d > 0 ascending by d, then i; c_j = 1 where entry i has bit 0 or bit 1 clear; C_j the inclusive prefix; J the first j
 *    with d_j > th_depth && C_j > 100, else the last pair; exactly the pairs j <= J with c_j = 1 get a point: position =
 *    csrc/keyframe_geom.h's back-projection on the last pose, flags 1, id -1, the feature's own descriptor.  TEMP_COUNT = C_J.
 *  2 Tcw (VO_TRACKER_TCW_START) = VELOCITY * last pose; VO_TRACKER_POSE_START = its se3 logarithm (:236).
 *  3 with ids on the local map AND the last list: link[j] = the lowest last index with local point j's id and bit 0 set, or -1,
 *    and the link is in force (:765).  Without ids on either side the link is left as it is.
 * vo_tracker_handover_arrays: the device addresses of SLOT_IDS, FRAME_POSE, MOTION_STATE (any pointer may be NULL), stable for
 * the tracker's life; no synchronisation.  vo_kfstore_keyframe_need_stats_dev / vo_kfstore_create_keyframe_from_frames take
 * dev_slot_ids and dev_Tcw12 from here.
 * The Tlr * ref pose refresh of :547-549: vo_tracker_record_ref_pose / vo_tracker_refresh_last_pose (below).
 * Not built: recoverLastFrame (replaced points), which needs a replacement log the store does not keep. */
typedef struct {
  float th_depth;      /* camera_->thDepth_ (:571) */
  int32_t min_tracked; /* <= 0: 30 (:310); read by vo_tracker_end_frame only */
} vo_tracker_handover_params;
int vo_tracker_set_last_frame_ids(vo_tracker *t, int n, const int32_t *ids /*[batch][n]*/);
int vo_tracker_set_last_pose(vo_tracker *t, const double *Tcw12 /*[batch][12]*/, const uint8_t *valid /*[batch]*/);
int vo_tracker_end_frame(vo_tracker *t, const vo_tracker_handover_params *p);
int vo_tracker_begin_frame(vo_tracker *t, const vo_tracker_handover_params *p, const uint8_t *dev_is_keyframe /*[batch] or NULL*/);
int vo_tracker_handover_arrays(vo_tracker *t, const int32_t **dev_slot_ids, const double **dev_Tcw12, const int32_t **dev_state);
/* The motion route from the key-frame store: with vo_tracker_build_local_map after
 * vo_tracker_track_first[_dev] (above), what a motion-tracked frame still took to the host -- the addVisible / addFound
 * counters of trackLocalMap and the Tlr * ref pose refresh of updateLastFrame --, so that a frame is one chain of enqueued calls:
 * begin_frame -> track_first_dev -> build_local_map(store) -> track_local_map -> point_stats -> end_frame -> record_ref_pose ->
 * ... -> refresh_last_pose -> begin_frame.  Their state is ONE device block of its own, allocated by the first call that needs
 * it (build_local_map on the motion route, or any of the four below): first slot ids 4 BF, a vote mask BF, three counter arrays
 * 3 x 4 B(F + M), Tcr 96 B, the key-frame numbers 4 B, and 8 BP sort keys of the link only where P > 4096 (B = batch, F =
 * max_features, M = max_local, P = the power of two >= max(F, max_last); every array rounded up to 4 KiB).  After that first call each is ENQUEUED on the tracker's stream: no allocation, no host synchronisation, no
 * device-to-host copy; the pose calls are ordered against the store's stream by events.  Every refusal happens before anything
 * is enqueued or any state changes.
 * vo_tracker_point_stats(): valid after vo_tracker_track_first[_dev] + vo_tracker_track_local_map with ids on the local map
 * (built, or vo_tracker_set_local_map_ids) and on the last-frame list; anything else VO_ERR_INVALID (the counters behind the
 * relocalisation and reference-key-frame routes: vo_tracker_point_stats_store, below).  One launch, a workgroup per frame, fills VO_TRACKER_STAT_IDS,
 * _VISIBLE and _FOUND, int32 [batch][max_features + max_local]:
 *  A entry i < max_features: p = the id slot i held when searchLocalMapPoints started -- VO_TRACKER_FIRST_SLOT_IDS[i] behind a
 *    built map; behind a local map the host set the same gather on the state as it stands (a slot the local search claimed
 *    counts as holding its last-frame entry, also where the first solve had culled it).  visible 1 (:738); found 1 iff the slot
 *    still holds that point (VO_TRACKER_ASSIGNED_LOCAL[i] < 0) and VO_TRACKER_FEATURE_OUTLIER[i] == 0 (:295-297).  p < 0 or
 *    i >= n: id -1, counts 0.  A map built on the motion route stays "the built map" of its frame until the next track call: a
 *    caller who replaces it through vo_tracker_set_local_map / _ids before vo_tracker_track_local_map still gets segment A from
 *    the build's FIRST_SLOT_IDS (its nulling has acted on the slots), and vo_tracker_results still reports the build's sticky word.
 *  B entry max_features + j: id = VO_TRACKER_LOCAL_POINT_IDS[j]; visible = bit 0 of VO_TRACKER_LOCAL_FLAGS[j] (:750-760); found 1
 *    iff the slot i with VO_TRACKER_ASSIGNED_LOCAL[i] == j has VO_TRACKER_FEATURE_OUTLIER[i] == 0.  Both counts 0: id -1.
 * vo_tracker_point_stats_arrays: the device addresses of the three arrays and their row length (any pointer may be NULL), stable
 * for the tracker's life; no synchronisation.  A frame's row goes straight into vo_kfstore_add_point_stats_dev(s, row_len, ...);
 * that call's bound n <= max_recent + max_features is the caller's to meet: max_recent >= max_local.
 * vo_tracker_record_ref_pose(store, dev_ref_kf [batch] or NULL) (:130-140): valid after vo_tracker_end_frame, before the next
 * track call or last-frame setter; the store needs vo_kfstore_enable_mapping (the pose column); else VO_ERR_INVALID.  Per frame
 * ref = dev_ref_kf[f] (NULL: VO_TRACKER_LOCAL_REF_KF[f]; VO_ERR_INVALID when no map was ever built) where it lies in [0, size) and
 * its pose is set, else the key-frame the frame remembers (:692-696).  With the frame's last pose valid and such a ref:
 * VO_TRACKER_REF_TCR = FRAME_POSE * pose(ref)^-1 and VO_TRACKER_REF_KF = ref; otherwise the previous pair stands (:138-139).
 * vo_tracker_refresh_last_pose(store) (:547-549): valid between vo_tracker_end_frame and vo_tracker_begin_frame, same store
 * condition; it is no last-frame setter: vo_tracker_begin_frame is accepted behind it.  A frame with a remembered pair: last
 * pose = REF_TCR * pose(REF_KF), its validity byte untouched; other frames are left alone.  vo_tracker_begin_frame then builds
 * the start pose and the temporary points on the refreshed pose (:549 before :581 and :236).  Inverse and product are
 * csrc/handover_geom.h's, every operation rounded.  One launch each. */
int vo_tracker_point_stats(vo_tracker *t);
int vo_tracker_point_stats_arrays(vo_tracker *t, const int32_t **dev_ids, const int32_t **dev_visible, const int32_t **dev_found,
                                  int32_t *row_len);
int vo_tracker_record_ref_pose(vo_tracker *t, const vo_kfstore *store, const int32_t *dev_ref_kf /*[batch] or NULL*/);
int vo_tracker_refresh_last_pose(vo_tracker *t, const vo_kfstore *store);
/* The hand-over and the counters behind the other two routes of VisualOdometry::run, which keep their
 * slot ids in the key-frame store: all three routes end in the same two enqueued calls, and relocalise -> reference key-frame
 * -> motion runs with no host array in between.  Both calls are valid only when ALL of these hold, else VO_ERR_INVALID:
 *  - the last front was vo_tracker_relocalize_store[_dev] / _db[_dev], or vo_tracker_track_ref_keyframe_store[_dev] with
 *    first_stage_only = 1;
 *  - this frame's local map was built by vo_tracker_build_local_map(store) (a map or ids set from the host since: refused);
 *  - vo_tracker_track_local_map has run behind the build.
 * One call is one route for the whole batch.  vo_tracker_end_frame and vo_tracker_point_stats stay refused behind these routes.
 * Each call is ONE launch, a workgroup per frame, ENQUEUED on the tracker's stream and ordered against the store's stream by
 * events as vo_tracker_build_local_map is (the observation index is rebuilt on the store's stream when stale): no host
 * synchronisation, no device-to-host copy, no allocation after the first call of the hand-over's / the counters' block.  They
 * have no state of their own.  Every refusal happens before anything is enqueued or any state changes.
 * vo_tracker_end_frame_store(store, p): max_features > max_last VO_ERR_CAPACITY.  Steps 2-5 and every output are
 * vo_tracker_end_frame's (SLOT_IDS, SLOT_DESC, FRAME_POSE, VELOCITY, MOTION_STATE, the last pose and its validity, the
 * rewritten last-frame list with ids, LAST_N = max_features); vo_tracker_begin_frame, _record_ref_pose, _refresh_last_pose,
 * _handover_arrays and the key-frame creation calls follow it as they follow vo_tracker_end_frame.  Step 1, slot i < n:
 *   relocalisation: a non-null slot (VO_TRACKER_FEATURE_HAS_POINT) carries VO_TRACKER_RELOC_POINT_IDS[i] (the local search's
 *    claims are in it already).  A frame whose relocalisation failed (VO_TRACKER_RELOC_WINNER < 0): every slot null, ok = 0, an
 *    empty list, the last pose invalid, MOTION_STATE 0 (:113-120, :128).
 *   reference key-frame: VO_TRACKER_ASSIGNED_LOCAL[i] = a1 >= 0 -> VO_TRACKER_LOCAL_POINT_IDS[a1]; else
 *    VO_TRACKER_ASSIGNED_LAST[i] = a0 >= 0 and the slot non-null -> the store's ids[ref_kf[f]][a0], the key-frame in [0, size)
 *    and a0 below its feature count; else null.
 *   both: an id < 0 is null.  observed = VO_TRACKER_FEATURE_OBSERVED[i], outlier = VO_TRACKER_FEATURE_OUTLIER[i], position =
 *    VO_TRACKER_FEATURE_POINTS[i].  Descriptor (mp->descriptor_) = the store's point descriptor at the id's first key of the
 *    observation index: the lowest (key-frame, feature) with flags bit 0 that holds the id, below size.
 *   DEVIATION: an id that no key-frame holds any more is a bad point (the reference would still hand the pointer over and skip
 *    it at its next use); the slot is handed over null.
 *   status and n_tracked of step 3 are those vo_tracker_results reports (the result block: on the relocalisation route they
 *    do not live in the tracker's own arrays); so is the pose of step 4.
 * vo_tracker_point_stats_store(store): fills the rows of vo_tracker_point_stats (same block, same addresses, straight into
 * vo_kfstore_add_point_stats_dev):
 *  A entry i < n: a non-null slot the local search did not claim (VO_TRACKER_ASSIGNED_LOCAL[i] < 0) counts with the id of the
 *    route's source above (RELOC_POINT_IDS[i], or the store's ids[ref_kf][a0]): visible 1 (:738), found 1 iff
 *    VO_TRACKER_FEATURE_OUTLIER[i] == 0 (:295-297).  Anything else: id -1, counts 0.
 *  B as vo_tracker_point_stats; VO_TRACKER_LOCAL_FLAGS are the flags isInFrame ran with on either route -- behind a
 *    relocalisation a local point the frame already holds was skipped by id and is not visible (:753).
 *  A frame whose relocalisation failed: a row of -1 / 0.
 * Not built: the host forms of the two routes and the one-call form of track_ref_keyframe_store (their local map is set by the
 * host); a batch whose frames take different routes (the caller groups streams); lastRelocateFrameId_; recoverLastFrame. */
int vo_tracker_end_frame_store(vo_tracker *t, vo_kfstore *store, const vo_tracker_handover_params *p);
int vo_tracker_point_stats_store(vo_tracker *t, vo_kfstore *store);
int vo_tracker_sync(vo_tracker *t);
/* HIP events on the launching streams around the six stages of every subsequent batch (bench.py):
 * 0 extraction, 1 frame post-processing, 2 search vs last frame, 3 pose solve + culling, 4 isInFrame +
 * search vs local map, 5 pose solve + count.  vo_tracker_get_timing synchronises, returns the summed
 * milliseconds since the last call and the number of timed batches, and resets. */
#define VO_TRACKER_STAGES 6
int vo_tracker_set_timing(vo_tracker *t, int enabled);
int vo_tracker_get_timing(vo_tracker *t, double *ms /*VO_TRACKER_STAGES*/, int *n_calls);

/* Optimizer::solveLoopSim3(keyframe_curr, keyframe_match, inlierMappoints, Scm, fixScaleFlag)
 * (optimizer_ceres.cpp:810-1030) with PoseOnlySim3 / PoseOnlyInverseSim3 (optimizer_ceres.h:211-267):
 * problem 1 (Huber sqrt(10), <= 10 iterations), chi2 > 10 rejection in both images, then 10 (or 5
 * when nothing was rejected) more iterations on the survivors and a final test of every match.
 * Batched: problem p owns matches offsets[p] .. offsets[p+1].  Per match: the map point in the
 * matched key-frame's camera frame (cam_match) with the current key-frame's pixel and 1/sigma, and
 * the current key-frame's camera-frame point (cam_curr) with the matched key-frame's pixel and
 * 1/sigma (:846-878).  poses[6p..] in/out = [angle-axis; t] of Scm, scales[p] its scale
 * (fix_scale: constant, loopClosing.cpp:15).  outlier[i] = 1: inlierMappoints entry nulled.
 * n_inliers[p] = return value; 0 with pose and scale untouched when fewer than 10 matches survive
 * problem 1 (:950-951).  summaries[2p].reserved reports the phase reached: 1 = returned after problem 1
 * (Scm must not be written), 2 = both problems ran (Scm = the result, even with 0 inliers). */
int vo_sim3_solve(int n_problems, const int32_t *offsets, const double *cam_match, const double *pix_curr,
                  const double *inv_sigma_curr, const double *cam_curr, const double *pix_match,
                  const double *inv_sigma_match, const double camera[4], int fix_scale, double *poses,
                  double *scales, uint8_t *outlier, int32_t *n_inliers, vo_lm_summary *summaries /*2 per problem or NULL*/);

/* The solve inside Optimizer::solvePoseGraphLoop (optimizer_ceres.cpp:1036-1305; cost functor
 * PoseGraphLoop, optimizer_ceres.h:269-325): key-frame i = Sim3 S_iw as unit quaternion quats[4i..]
 * (Eigen coefficient order x, y, z, w; ceres::EigenQuaternionParameterization), translation
 * trans[3i..], scale scales[i] (constant: fix_scale must be 1, as loopClosing.cpp:15 always passes);
 * edge e (edge_i -> edge_j) measures S_ji = (q_meas, t_meas, s_meas) (:1094-1236).  fixed_node is
 * keyframe_match (:1238-1240).  No loss, LM, exact solve of the normal equations
 * (SPARSE_NORMAL_CHOLESKY in the reference; here a dense blocked Cholesky with the trailing update on
 * the FP64 matrix cores), max_iterations = 20 in the reference (:1253).  6 * (nodes - 1) <= 4096. */
int vo_pose_graph_solve(int n_nodes, double *quats, double *trans, const double *scales, int fixed_node,
                        int n_edges, const int32_t *edge_i, const int32_t *edge_j, const double *q_meas,
                        const double *t_meas, const double *s_meas, int fix_scale, int max_iterations,
                        vo_lm_summary *summary);

/* Map-point re-anchoring after the pose graph (optimizer_ceres.cpp:1281-1301):
 * out = S_wr[ref] * (S_rw[ref] * p); a Sim3 is 8 doubles: quaternion (x, y, z, w), translation, scale.
 * ref_node[i] < 0 leaves the point unchanged (bad points are skipped, :1284-1285). */
int vo_sim3_reanchor_points(int n_points, const double *points_in, const int32_t *ref_node, int n_nodes,
                            const double *S_rw, const double *S_wr, double *points_out);

/* Dense symmetric positive definite solve on the device (the blocked Cholesky behind
 * vo_pose_graph_solve): A row-major, lower triangle read and overwritten by its factor, b -> x. */
int vo_chol_solve(int n, double *A_rowmajor_lower, double *b);

/* The same solve through the split (per-rank segment) form that a sharded global BA can use (vo_ba_set_shard +
 * vo_ba_set_allreduce with VO_BA_OPT_SEGMENTS), with the n_ranks shards
 * emulated one after the other on this GPU -- a test entry: the 64-column tile columns [0, c0_tiles) hold segments that
 * are independent of each other (col_part[j] = the segment of tile column j, owned by rank col_part[j] % n_ranks), the
 * remaining tile columns the separators.  Per rank: eliminate the own segments into the separator block; the separator
 * blocks are summed (the all-reduce); every rank solves the separators and substitutes back into its segments.  b -> x. */
int vo_chol_solve_split(int n, const double *A_rowmajor_lower, double *b, int c0_tiles, const int32_t *col_part, int n_ranks);

/* Bundle-adjustment problem handle (the arrays Optimizer::solveLocalBAPoseAndPoint gathers at
 * optimizer_ceres.cpp:446-592).  Edges may be given in any order; they are grouped by point
 * internally (stable).  cam_fixed[c] != 0 <=> SetParameterBlockConstant (:578-579). */
typedef struct vo_ba vo_ba;
int vo_ba_create(vo_ba **out, int n_cams, const double *poses, const uint8_t *cam_fixed, int n_points,
                 const double *points, int n_edges, const int32_t *edge_cam,
                 const int32_t *edge_point, const double *edge_obs, const double *edge_inv_sigma,
                 const double cam[5]);
void vo_ba_destroy(vo_ba *h);
/* A NEW problem in an existing handle: the per-key-frame caller (localMapping.cpp:38 builds a different local window every
 * time) keeps ONE handle per thread and resets it instead of create / destroy -- stream, device buffers (grow-only, with
 * headroom), page-locked staging, shard / callback / options stay, so that nothing is allocated or freed on the hot path
 * (hipFree synchronises the whole device, the tracking thread's streams included).  Arguments as vo_ba_create.  Caller-owned
 * reduce buffers (vo_ba_set_reduce_buffers) were sized for the previous problem: the reset forgets them, set them again.  A
 * problem that is rejected (VO_ERR_INVALID: an edge out of range) leaves the handle's previous problem in place. */
int vo_ba_reset(vo_ba *h, int n_cams, const double *poses, const uint8_t *cam_fixed, int n_points, const double *points,
                int n_edges, const int32_t *edge_cam, const int32_t *edge_point, const double *edge_obs,
                const double *edge_inv_sigma, const double cam[5]);
int vo_ba_set_stream(vo_ba *h, void *hip_stream);
/* restrict this handle to the points p with p % n_shards == shard (multi-GPU: one process per
 * GPU, each owning a shard; cameras replicated).  Must precede any solve.
 * (With VO_BA_OPT_SEGMENTS set, an all-reduce callback and a large reduced system whose key-frame order has
 * nested-dissection segments, a point belongs to the rank of the segment it touches instead -- see vo_ba_set_allreduce.) */
int vo_ba_set_shard(vo_ba *h, int shard, int n_shards);
/* Per-handle options; must precede the first use of the handle (any solve, vo_ba_set_state, vo_ba_debug_order) and be the
 * same on every rank of a sharded solve.  A sharded handle with an all-reduce callback checks that with one small
 * handshake all-reduce when it is first used: ranks that disagree on the options, the shard count or the problem fail
 * with VO_ERR_INVALID instead of waiting for each other in mismatched collectives.
 *   VO_BA_OPT_SEGMENTS                 1: per-rank segment factorisation (see vo_ba_set_allreduce); default 0
 *   VO_BA_OPT_COLLECTIVES_AT_ONE_RANK  1: a handle of ONE shard with a callback runs the sharded form of the loop (for
 *                                      bringing a collective up on a one-GPU machine: every call is a sum over one rank)
 *   VO_BA_OPT_ORDER_PARTS              force the number of nested-dissection parts of a large system's key-frame order
 *                                      (1 = natural order; -1 = choose, the default) */
enum { VO_BA_OPT_SEGMENTS = 1, VO_BA_OPT_COLLECTIVES_AT_ONE_RANK = 2, VO_BA_OPT_ORDER_PARTS = 3 };
int vo_ba_set_option(vo_ba *h, int option, int value);
/* Process-wide developer knobs: VO_OPT_BA_GRAPH 1 = replay the LM iteration sequence of an unsharded solve from a
 * hipGraph (default 0: eager launches are faster on this stack); VO_OPT_POSE_BLOCK = threads per
 * frame of the pose-only solver (0 = automatic, 64, 128, 256); VO_OPT_HAMMING_KERNEL = which form of the all-pairs Hamming
 * kernel vo_hamming_matrix* launch: 0 (default) = int8 matrix-core dot products, 1 = the xor / popcount VALU form (identical
 * results); VO_OPT_BA_PAIRS_KERNEL = which kernel gathers the reduced camera system of a LARGE problem
 * (more than 21 free key-frames): 0 (default) = k_ba_pairs_lds, blocks staged through LDS, 1 = k_ba_pairs, lane = couple (the two
 * agree to rounding, not bitwise: the order of the sums differs). */
enum { VO_OPT_BA_GRAPH = 1, VO_OPT_POSE_BLOCK = 2, VO_OPT_HAMMING_KERNEL = 3, VO_OPT_BA_PAIRS_KERNEL = 4 };
int vo_set_option(int option, int value);
/* Multi-GPU from C/C++: the all-reduce the sharded LM loop needs (sum of n doubles at dev_buf over all
 * shards, in place, ordered on hip_stream; returns 0).  With RCCL this is
 *   ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, comm, (hipStream_t)stream)
 * over xGMI.  Once set, vo_ba_solve / vo_ba_local_ba[_enqueue] on a sharded handle run the whole LM
 * schedule with exactly two calls of it per iteration (the reduced camera system, 6 scalars); every
 * rank must make the same calls.  Without it those entry points reject a sharded handle
 * (VO_ERR_INVALID) instead of solving from partial sums.
 * Per-rank segment factorisation (opt-in, vo_ba_set_option(h, VO_BA_OPT_SEGMENTS, 1); large reduced systems only): every rank eliminates the
 * nested-dissection segments it owns, and the calls per iteration become four -- the camera-block extras, the separator
 * block after the elimination, the step, 6 scalars; vo_ba_linearize / vo_ba_step refuse such a handle.  The option
 * takes effect when the handle is first used and must be the same on every rank (checked by a handshake).  Measured with
 * emulated ranks it does more work per rank than the default, which is why it is not the default.
 * VO_BA_OPT_COLLECTIVES_AT_ONE_RANK: a handle of ONE shard with a callback runs the same sharded form of the loop (for
 * bringing a collective up on a one-GPU machine: every call is a sum over one rank; tests/test_gpu_rccl.py). */
typedef int (*vo_allreduce_fn)(void *user, double *dev_buf, size_t n_doubles, void *hip_stream);
int vo_ba_set_allreduce(vo_ba *h, vo_allreduce_fn fn, void *user);
int vo_ba_set_state(vo_ba *h, const double *poses, const double *points);
int vo_ba_get_state(vo_ba *h, double *poses, double *points);
int vo_ba_n_free_cams(const vo_ba *h);
/* The key-frame order a large reduced system (6 nf + 1 > 128) is factored in, chosen when the handle is first used:
 * out = {parts, cyclic, separator key-frames, dependent tile columns on the longest chain, tiles of L, tile rows,
 * tile products L(i,k) L(j,k)^T of the factorisation (2 x 64^3 flop each), first separator tile column of a handle in
 * segment mode or 0}; parts == 1: the natural order.
 * (Tests and tools; all zero tile rows for LDS-sized systems.) */
int vo_ba_debug_order(vo_ba *h, int out[8]);

/* Full Optimizer::solveLocalBAPoseAndPoint numerics (:530-755): Huber LM (5 iterations), float
 * chi2 classification, plain LM (10 iterations) on the inliers, final chi2 pass.
 * stop: NULL or the address of the reference's LIVE `bool stopFlag` (read as a byte, so a C++ caller passes
 * reinterpret_cast<const volatile unsigned char *>(&stopFlag)), polled exactly at :594 and :612.
 * edge_erase[n_edges] (host) out in the caller's edge order.  summaries: NULL or [2]. */
int vo_ba_local_ba(vo_ba *h, const volatile unsigned char *stop, uint8_t *edge_erase,
                   vo_lm_summary *summaries);
/* The same schedule split into "queue everything on the handle's stream" and "wait + fetch results",
 * so that several independent problems (handles) overlap on one GPU. */
int vo_ba_local_ba_enqueue(vo_ba *h, const volatile unsigned char *stop);
int vo_ba_local_ba_finish(vo_ba *h, uint8_t *edge_erase, vo_lm_summary *summaries);
/* The same for a key-frame of a store, gathered and written back on the device (the contract: the vo_kfstore block above). */
int vo_kfstore_local_ba(vo_kfstore *s, vo_ba *ba, int current, const volatile unsigned char *stop, vo_lm_summary *summaries);
/* One Ceres-style LM solve (ceres::Solve with DENSE_SCHUR at :604 / :699) on the current state.
 * huber_* <= 0 disables the loss.  edge_active: NULL or host mask in caller's edge order. */
int vo_ba_solve(vo_ba *h, double huber_mono, double huber_stereo, int max_iterations,
                const uint8_t *edge_active, vo_lm_summary *summary);

/* Split-phase interface used by the multi-GPU driver and the kernel-level tests:
 *   vo_ba_linearize   evaluate residuals/Jacobians at the current state, assemble the point
 *                     blocks and this shard's contribution to the reduced camera system into the
 *                     device buffer returned by vo_ba_reduced_system(): packed doubles
 *                     [ S (6nf x 6nf row-major) | b (6nf) | cost | |x|^2 ... ] -- the buffer that is
 *                     all-reduced (sum) across shards each LM iteration.
 *   vo_ba_step        Cholesky-solve the (already reduced) system, back-substitute, form the
 *                     candidate state, evaluate its cost -> second small reduced buffer.
 *   vo_ba_update      accept / reject, trust-region radius update, convergence flags.
 * All three are asynchronous on the handle's stream; no host synchronisation inside. */
int vo_ba_lm_begin(vo_ba *h, double huber_mono, double huber_stereo, int max_iterations,
                   const uint8_t *edge_active);
int vo_ba_linearize(vo_ba *h);
int vo_ba_step(vo_ba *h);
int vo_ba_update(vo_ba *h);
int vo_ba_lm_end(vo_ba *h, vo_lm_summary *summary);
/* let the caller own the two all-reduce payload buffers (e.g. torch tensors handed to
 * torch.distributed); sizes as reported by vo_ba_reduced_system / vo_ba_reduced_cost.
 * Must precede vo_ba_lm_begin; vo_ba_reset forgets them (they are sized by the problem). */
int vo_ba_set_reduce_buffers(vo_ba *h, double *dev_system, double *dev_cost);
/* device pointers + element counts of the two all-reduce payloads */
int vo_ba_reduced_system(vo_ba *h, double **dev_ptr, size_t *n_doubles);
int vo_ba_reduced_cost(vo_ba *h, double **dev_ptr, size_t *n_doubles);
/* pieces of the local-BA schedule for drivers that run the LM loop themselves (multi-GPU):
 *   vo_ba_classify(h, 0)  float chi2 test of optimizer_ceres.cpp:618-689 on the current state; the
 *                         device-side edge mask becomes "inlier", outliers are remembered
 *   vo_ba_lm_begin_inliers  like vo_ba_lm_begin but keeps that device-side mask (problem 2, :691-699)
 *   vo_ba_classify(h, 1)  final pass :703-755 (adds to the remembered outliers)
 *   vo_ba_get_edge_outliers  the remembered mask in the caller's edge order (edgeErase) */
int vo_ba_classify(vo_ba *h, int final_pass);
int vo_ba_lm_begin_inliers(vo_ba *h, double huber_mono, double huber_stereo, int max_iterations);
int vo_ba_get_edge_outliers(vo_ba *h, uint8_t *edge_erase);
/* copy out the undamped reduced camera system of the current linearisation (tests):
 * S [6nf*6nf], b [6nf], cost.  point_damping is added to every point-block diagonal. */
int vo_ba_debug_schur(vo_ba *h, double huber_mono, double huber_stereo, double point_damping,
                      const uint8_t *edge_active, double *S, double *b, double *cost);

/* Developer instrumentation: s_memrealtime stamps (100 MHz ticks) written by the BA kernels of a
 * -DVO_BA_STAMPS build (tools/ba_stamps.py); all zero in the product build.  out[48]. */
int vo_ba_debug_stamps(vo_ba *h, unsigned long long *out);

/* SE3 helpers the shims need (Sophus SE3::exp / log as used at :163,:257,:474,:787) */
int vo_se3_exp(const double xi[6], double R_rowmajor[9], double t[3]);
int vo_se3_log(const double R_rowmajor[9], const double t[3], double xi[6]);

#ifdef __cplusplus
}
#endif
#endif /* VO_HIP_H */
