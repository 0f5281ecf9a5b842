// tracker.hip -- the tracked-frame pipeline behind the C-ABI (vo_tracker_*): what VisualOdometry::trackWithMotion +
// trackLocalMap do per frame (reference src/visualOdometry.cpp:228-251, 286-300, 745-775, 864-886), for a batch of
// independent camera streams that stay in HBM from the image to the pose:
//
//   ORB extraction (frame.cpp:22)                    vo_orb_extract_batch_dev          extraction stream
//   Frame::Frame post-processing, grid (:27-32)      vo_frames_build_dev               tracking stream from here on
//   searchByProjection(frame, last frame, 15)        k_track_project_prep + vo_match_guided_dev mode 0 (+ the 2 x radius retry)
//   solvePoseOnlySE3                                 k_track_scatter_gather (the matches into the frame's slots, the
//                                                    observation list) + k_pose_only
//   cullingOutliersBeforeLocalMap (:864-886)         k_track_cull: outliers of the solve lose their map point
//   searchLocalMapPoints: Frame::isInFrame (frame.cpp:145-190, with the REFINED pose) + MapPoint::predictScale
//                                                    k_track_in_frame
//   searchByProjection(frame, local points, 3)       vo_match_guided_dev mode 1
//   solvePoseOnlySE3, inlier count (:289-300)        k_track_scatter_gather + k_pose_only + k_track_count (which also
//                                                    writes the frame's record of the result block)
//
// trackRefKeyFrame (:256-277) replaces the projection search by searchByBoW(reference key-frame, frame): stage_ref_keyframe (key-frames
// from host arrays, the common-node walk on the host) or stage_ref_keyframe_store (key-frames read from a vo_kfstore by
// number: k_featvec, k_ref_kf_gather, k_bow_walk, k_node_replay -- launches only).
//
// 27 kernel launches per batch (round 4: 33), no host synchronisation in between.  The extraction may run on a stream shared by several
// trackers (vo_tracker_config.extract_stream): batch i + 1's extraction then overlaps batch i's searches and pose
// solves (two events order them).  Round 2 kept this sequence in Python (vo_slam_test_amd/tracking.py) without the
// culling step and with the local-map projections fixed before the first solve; host code is now C++
// throughout, as the reference's callers are.
#include "tracker_state.h"

#include <cmath>
#include <new>
#include <vector>

#include "ba_math.h"

namespace {

using namespace vo;
using namespace vo::ba;

// Start of a tracked batch: the feature -> map-point state of every frame is cleared and the solver's pose starts at the
// motion-model pose -- one launch instead of four memsets and a copy (a launch or a copy costs ~5 us of a 0.7 ms frame
// when one camera stream is tracked at a time).
__global__ __launch_bounds__(256) void k_track_prep(int cap, int last_stride, int *assigned, uint8_t *fhas, uint8_t *fobs,
                                                    uint8_t *last_matched, const double *pose0, double *pose) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const long long o = (long long)f * cap;
  for (int i = tid; i < cap; i += 256) assigned[o + i] = -1, fhas[o + i] = 0, fobs[o + i] = 0;
  for (int i = tid; i < last_stride; i += 256) last_matched[(long long)f * last_stride + i] = 0;
  if (tid < 6) pose[6 * f + tid] = pose0[6 * f + tid];
}

// k_track_prep and the projection prologue of searchByProjection(Frame*, Frame*) (k_track_project, csrc/track.hip: the
// same arithmetic, matcher.cpp:41-64) in one launch: the two touch disjoint arrays.  Block (x, f) projects queries
// [256 x, 256 x + 256) of frame f and clears the slice of the per-feature state that the blocks of a frame share out.
__global__ __launch_bounds__(256) void k_track_project_prep(int nq, int stride, const double *Tcw, const double *points,
                                                            const uint8_t *pflags, float fx, float fy, float cx, float cy, int xmin,
                                                            int xmax, int ymin, int ymax, uint8_t *qflags, float *qu, float *qv,
                                                            float *qinvz, int cap, int *assigned, uint8_t *fhas, uint8_t *fobs,
                                                            uint8_t *last_matched, const double *pose0, double *pose) {
  const int f = blockIdx.y, tid = threadIdx.x, q = blockIdx.x * 256 + tid;
  {
    const long long o = (long long)f * cap;
    const int step = (int)gridDim.x * 256;
    for (int i = q; i < cap; i += step) assigned[o + i] = -1, fhas[o + i] = 0, fobs[o + i] = 0;
    for (int i = q; i < stride; i += step) last_matched[(long long)f * stride + i] = 0;
    if (blockIdx.x == 0 && tid < 6) pose[6 * f + tid] = pose0[6 * f + tid];
  }
  if (q >= nq) return;
  const long long o = (long long)f * stride + q;
  const double *T = Tcw + 12 * (long long)f, *p = points + 3 * o;
  const unsigned pf = pflags[o];
  uint8_t out = 0;
  float u = 0.f, v = 0.f, invz = 0.f;
  if (pf & 1u) {
    const double x = T[0] * p[0] + T[1] * p[1] + T[2] * p[2] + T[9];
    const double y = T[3] * p[0] + T[4] * p[1] + T[5] * p[2] + T[10];
    const double zc = T[6] * p[0] + T[7] * p[1] + T[8] * p[2] + T[11];
    const float z = (float)zc;
    if (!(z < 0.0f)) {  // :52-53
      invz = 1.0f / z;
      u = (float)((double)fx * x / zc + (double)cx);  // Camera::camera2pixel, camera.cpp:72-75 (float members widened)
      v = (float)((double)fy * y / zc + (double)cy);
      if (!(u < xmin || u > xmax) && !(v < ymin || v > ymax)) out = (uint8_t)(1u | (pf & 2u));  // :61-64
    }
  }
  qflags[o] = out, qu[o] = u, qv[o] = v, qinvz[o] = invz;
}

// End of a batch: everything vo_tracker_results hands back -- pose, the four counts, the status word per frame, and the
// two stages' sticky overflow flags -- in one block, so that the host needs ONE download (it was eight small ones and
// three synchronisations: ~60 us of a 0.7 ms frame).  Record: [pose 6 doubles | n_tracked, n_inliers, n_matches_last,
// n_matches_local, status, 0] = 72 bytes; the flags follow the records.
struct PackArgs {
  int B;
  const double *pose;
  const int *ninl, *nm_first, *nm, *orb_err, *guided_err;
  uint8_t *out;
  const int *store_err;  // the store routes' sticky word, or NULL on a route that reads no store (the third flag stays)
};
__device__ __forceinline__ void pack_record(const PackArgs &K, int f, int ntracked, int status) {
  double *pd = reinterpret_cast<double *>(K.out + (size_t)f * 72);
  for (int k = 0; k < 6; k++) pd[k] = K.pose[6 * f + k];
  int *pi = reinterpret_cast<int *>(K.out + (size_t)f * 72 + 48);
  pi[0] = ntracked, pi[1] = K.ninl[f], pi[2] = K.nm_first[f], pi[3] = K.nm[f], pi[4] = status, pi[5] = 0;
  if (f == 0) {
    int *fl = reinterpret_cast<int *>(K.out + (size_t)K.B * 72);
    fl[0] = K.orb_err ? *K.orb_err : 0;
    fl[1] = K.guided_err ? *K.guided_err : 0;
    if (K.store_err) fl[2] = *K.store_err;
  }
}
// (on its own: the first frame of a sequence, whose counts are memsets)
__global__ __launch_bounds__(256) void k_track_pack(PackArgs K, const int *ntracked, const int *status) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < K.B) pack_record(K, f, ntracked[f], status[f]);
}

// cullingOutliersBeforeLocalMap (visualOdometry.cpp:864-886) on the pose solver's observation list: an outlier's
// feature loses its map point (`mappoints_[i] = nullptr`, and with it the "holds an observed point" mark the local-map
// search tests at matcher.cpp:314); inliers whose point has observations are counted (the function's return value).
// Also marks the last-frame points that were matched at all: matched points -- kept or culled -- carry
// visualIdxOfFrame_ == frame id (:752, :881) and are skipped by searchLocalMapPoints (:765).
// It also keeps the first search's assignments, pose and inlier count for the caller (VO_TRACKER_*_FIRST) and hands
// `assigned` to the second search cleared -- three copies and a memset less per batch.
struct CullArgs {
  int cap;
  const int *ranges, *index;
  const uint8_t *outlier;
  int *assigned;
  int last_stride;
  uint8_t *fhas, *fobs, *last_matched;
  int *n_observed_inliers, *assigned_first;
  const double *pose;
  double *pose_first;
  const int *ninl;
  int *ninl_first;
};
__device__ __forceinline__ void cull_frame(const CullArgs &C, int f, int *s_cnt) {
  const int tid = threadIdx.x;
  const long long o = (long long)f * C.cap;
  const int start = C.ranges[2 * f], count = C.ranges[2 * f + 1];
  for (int i = tid; i < C.cap; i += 256) {
    const int a = C.assigned[o + i];
    if (a >= 0) C.last_matched[(long long)f * C.last_stride + a] = 1;
    C.assigned_first[o + i] = a;
    C.assigned[o + i] = -1;
  }
  if (tid < 6) C.pose_first[6 * f + tid] = C.pose[6 * f + tid];
  if (tid == 6) C.ninl_first[f] = C.ninl[f];
  int local = 0;
  for (int d = tid; d < count; d += 256) {
    const int i = C.index[start + d];
    if (C.outlier[start + d]) {
      C.fhas[o + i] = 0;
      C.fobs[o + i] = 0;
    } else if (C.fobs[o + i]) {
      local++;
    }
  }
  for (int s = 32; s >= 1; s >>= 1) local += __shfl_xor(local, s);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) C.n_observed_inliers[f] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}
__global__ __launch_bounds__(256) void k_track_cull(CullArgs C) {
  __shared__ int s_cnt[4];
  cull_frame(C, blockIdx.x, s_cnt);
}
// Frame::isInFrame (frame.cpp:145-190) and MapPoint::predictScale (mappoint.cpp:182-196) for the local map points of
// every frame, with Tcw = exp(pose) of the first solve (frame->setPose, optimizer_ceres.cpp:311).  Arithmetic as the
// reference has it: the transform in double (Sophus SE3 * Vector3d = Eigen's quaternion rotation), z, u, v, the
// distance and the view cosine narrowed to float where the reference narrows them, logf as the correctly rounded
// float of the double logarithm (the reference calls glibc's logf: DESIGN section 3).
// pflags bit 0: the point exists, is not bad and is not already in the frame; bit 1: it has observations.
struct InFrameArgs {
  int nq, stride;
  const double *pose6, *points, *normals;
  const float *min_dist, *max_dist;
  const uint8_t *pflags;
  const int *link;
  const uint8_t *last_matched;
  int last_stride;
  float fx, fy, cx, cy, bf, xmin, xmax, ymin, ymax, log_sf1;
  int n_levels;
  uint8_t *qflags;
  float *qu, *qv, *qur;
  int *qlevel;
  float *qviewcos;
  const int *frame_on;  // [frames] or NULL: a negative entry leaves the frame out (nothing of it is written)
};
// s_T: q (w, x, y, z), t, Ow of the frame's pose (in_frame_pose), set by one thread before a barrier
__device__ __forceinline__ void in_frame_pose(const InFrameArgs &A, int f, double *s_T) {
  const Se3 T = se3_exp(A.pose6 + 6 * (long long)f);
  // Ow_ = Tcw.inverse().translation() (frame.cpp:103): the conjugate rotation of -t
  const double qc[4] = {T.q[0], -T.q[1], -T.q[2], -T.q[3]}, nt[3] = {-T.t[0], -T.t[1], -T.t[2]};
  double ow[3];
  quat_rotate(qc, nt, ow);
  for (int k = 0; k < 4; k++) s_T[k] = T.q[k];
  for (int k = 0; k < 3; k++) s_T[4 + k] = T.t[k], s_T[7 + k] = ow[k];
}
__device__ __forceinline__ void in_frame_query(const InFrameArgs &A, int f, int q, const double *s_T) {
  const long long o = (long long)f * A.stride + q;
  const unsigned pf = A.pflags[o];
  uint8_t out = 0;
  float u = 0.f, v = 0.f, ur = 0.f, vc = 0.f;
  int level = 0;
  const int lk = A.link ? A.link[o] : -1;
  const bool in_frame_already = lk >= 0 && A.last_matched[(long long)f * A.last_stride + lk] != 0;  // :765
  if ((pf & 1u) && !in_frame_already) {
    const double *p = A.points + 3 * o, *nv = A.normals + 3 * o;
    const double qq[4] = {s_T[0], s_T[1], s_T[2], s_T[3]};
    double rp[3];
    quat_rotate(qq, p, rp);
    const double x = rp[0] + s_T[4], y = rp[1] + s_T[5], zc = rp[2] + s_T[6];
    const float z = (float)zc;
    if (!(z < 0.0f)) {  // :153-154
      u = (float)((double)A.fx * x / zc + (double)A.cx);  // Camera::camera2pixel, camera.cpp:72-75 (float members widened)
      v = (float)((double)A.fy * y / zc + (double)A.cy);
      if (!(u < A.xmin || u > A.xmax) && !(v < A.ymin || v > A.ymax)) {  // :159-164
        const double l0 = p[0] - s_T[7], l1 = p[1] - s_T[8], l2 = p[2] - s_T[9];
        const float dist = (float)sqrt(l0 * l0 + l1 * l1 + l2 * l2);  // :167
        const float mind = 0.8f * A.min_dist[o], maxd = 1.2f * A.max_dist[o];  // mappoint.cpp:391-401
        if (!(dist < mind || dist > maxd)) {
          vc = (float)(l0 * nv[0] + l1 * nv[1] + l2 * nv[2]) / dist;  // :176
          if (!(vc < 0.5f)) {
            out = (uint8_t)(1u | (pf & 2u));
            ur = u - A.bf / z;  // :184
            const float ratio = A.max_dist[o] / dist;  // mappoint.cpp:187
            const float lg = (float)log((double)ratio);
            const int s = (int)ceilf(lg / A.log_sf1);
            level = s < 0 ? 0 : (s >= A.n_levels ? A.n_levels - 1 : s);
          }
        }
      }
    }
  }
  if (!out) u = v = ur = vc = 0.f, level = 0;
  A.qflags[o] = out, A.qu[o] = u, A.qv[o] = v, A.qur[o] = ur, A.qlevel[o] = level, A.qviewcos[o] = vc;
}
__global__ __launch_bounds__(256) void k_track_in_frame(InFrameArgs A) {
  __shared__ double s_T[10];
  const int f = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  if (A.frame_on && A.frame_on[f] < 0) return;
  if (threadIdx.x == 0) in_frame_pose(A, f, s_T);
  __syncthreads();
  if (q < A.nq) in_frame_query(A, f, q, s_T);
}
// trackLocalMap's inlier count (visualOdometry.cpp:289-300): features that hold a map point with observations and are
// no outlier of the second solve; and the per-frame status word.
__global__ __launch_bounds__(256) void k_track_count(int cap, const int *ranges, const int *index, const uint8_t *outlier,
                                                     const uint8_t *fobs, const int *n_first, const int *n_observed_first,
                                                     const int *ninl_first, int *n_tracked, int *status, int min_matches,
                                                     uint8_t *feature_outlier, PackArgs K) {
  __shared__ int s_cnt[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  const long long o = (long long)f * cap;
  const int start = ranges[2 * f], count = ranges[2 * f + 1];
  // frame_curr_->outliers_[i] after the second solve, per feature (features without a map point: 0)
  for (int i = tid; i < cap; i += 256) feature_outlier[o + i] = 0;
  __syncthreads();
  int local = 0;
  for (int d = tid; d < count; d += 256) {
    if (outlier[start + d]) feature_outlier[o + index[start + d]] = 1;
    if (!outlier[start + d] && fobs[o + index[start + d]]) local++;
  }
  for (int s = 32; s >= 1; s >>= 1) local += __shfl_xor(local, s);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) {
    const int n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    n_tracked[f] = n;
    int st = 0;
    if (n_first[f] < min_matches) st |= VO_TRACK_FEW_MATCHES;      // visualOdometry.cpp:247-248 (20) / :268-269 (15)
    if (n_observed_first[f] < 10) st |= VO_TRACK_FEW_INLIERS;      // :253
    (void)ninl_first;
    status[f] = st;
    pack_record(K, f, n, st);  // the frame's record of the result block (was a launch of its own)
  }
}

// status word and counts after the first stage alone (vo_tracker_track_first): what trackWithMotion / trackRefKeyFrame
// return -- enough matches, and at least 10 observed inliers after the culling (:247-253, :268-275)
__global__ __launch_bounds__(256) void k_track_first_status(int B, const int *n_first, const int *n_observed_first, int *n_tracked,
                                                            int *status, int min_matches, PackArgs K) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= B) return;
  int st = 0;
  if (n_first[f] < min_matches) st |= VO_TRACK_FEW_MATCHES;
  if (n_observed_first[f] < 10) st |= VO_TRACK_FEW_INLIERS;
  n_tracked[f] = n_observed_first[f];
  status[f] = st;
  pack_record(K, f, n_observed_first[f], st);
}

// trackRefKeyFrame from the key-frame store (vo_tracker_track_ref_keyframe_store): what vo_tracker_set_ref_keyframe uploads,
// read out of the store instead.  Frame f's reference key-frame is record ref_kf[f]: its `points` section into p0 and its
// `flags` section into pf0 and q0_flags (row stride n_last, zero beyond the key-frame's n), so that the tail of the
// pipeline indexes them exactly as after the host call.  One lane per double of the points section -- 24 bytes per
// feature, the section contiguous per key-frame: consecutive lanes read and write consecutive doubles -- and the first
// n_last lanes of a frame also copy a flag byte each.  Thread 0 of a frame's first block writes the start pose: Tcw as
// given and its se3 logarithm (frame_curr_->setPose(frame_last_->Tcw_), :259).  A number outside [0, size) is a key-frame
// without features and raises the store routes' sticky word (only ever OR-ed).
__global__ __launch_bounds__(256) void k_ref_kf_gather(vo::KfStoreView S, const int *ref_kf, const double *Tcw_in, int n_last,
                                                       double *p0, uint8_t *pf0, uint8_t *q0_flags, double *Tcw, double *pose0,
                                                       int *err) {
  const int f = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  const int k = ref_kf[f];
  const bool have = k >= 0 && k < S.size;
  const int n = have ? min(max(vo::kf_head(S, k)[0], 0), min(S.NK, n_last)) : 0;
  if (j == 0) {
    if (!have) atomicOr(err, (int)vo::kStoreErrBadId);
    const double *T = Tcw_in + 12 * (size_t)f;
    for (int i = 0; i < 12; i++) Tcw[12 * (size_t)f + i] = T[i];
    double xi[6];
    se3_log_from_R(T, T + 9, xi);
    for (int i = 0; i < 6; i++) pose0[6 * (size_t)f + i] = xi[i];
  }
  const size_t o = (size_t)f * n_last;
  if (j < 3 * n_last) p0[3 * o + j] = j < 3 * n ? vo::kf_sec<double>(S, k, S.o_points)[j] : 0.0;
  if (j < n_last) {
    const uint8_t fl = j < n ? vo::kf_sec<uint8_t>(S, k, S.o_flags)[j] : (uint8_t)0;
    pf0[o + j] = fl, q0_flags[o + j] = fl;
  }
}

constexpr int kStages = VO_TRACKER_STAGES;

}  // namespace

void vo_tracker::layout(vo::Arena &a) {
  const size_t B = this->B, nl = (size_t)n_last, nm = (size_t)n_local, cap = this->cap;
  a.take(d.cnt, B * 4 + 64);
  a.take(d.q0_flags, B * nl);
  a.take(d.q0_u, B * nl * 4);
  a.take(d.q0_v, B * nl * 4);
  a.take(d.q0_aux, B * nl * 4);
  a.take(d.q0_level, B * nl * 4);
  a.take(d.q0_angle, B * nl * 4);
  a.take(d.q0_desc, B * nl * 32);
  a.take(d.p0, B * nl * 24);
  a.take(d.pf0, B * nl);
  a.take(d.last_matched, B * nl + 64);
  a.take(d.q1_flags, B * nm);
  a.take(d.q1_u, B * nm * 4);
  a.take(d.q1_v, B * nm * 4);
  a.take(d.q1_aux, B * nm * 4);
  a.take(d.q1_level, B * nm * 4);
  a.take(d.q1_viewcos, B * nm * 4);
  a.take(d.q1_desc, B * nm * 32);
  a.take(d.p1, B * nm * 24);
  a.take(d.nrm1, B * nm * 24);
  a.take(d.mind1, B * nm * 4);
  a.take(d.maxd1, B * nm * 4);
  a.take(d.pf1, B * nm);
  a.take(d.link1, B * nm * 4);
  a.take(d.ids1, B * nm * 4);
  a.take(d.Tcw, B * 96 + 64);  // Tcw, then the intrinsics as doubles
  a.take(d.pose0, B * 48);
  a.take(d.pose, B * 48);
  a.take(d.pose_first, B * 48);
  a.take(d.resblk, B * 72 + 64);
  a.take(d.assigned, B * cap * 4);
  a.take(d.assigned_first, B * cap * 4);
  a.take(d.nm, B * 4 + 64);
  a.take(d.nm_first, B * 4 + 64);
  a.take(d.fpoint, B * cap * 24);
  a.take(d.fhas, B * cap);
  a.take(d.fobs, B * cap);
  a.take(d.pts, B * cap * 24);
  a.take(d.obs, B * cap * 24);
  a.take(d.isg, B * cap * 8);
  a.take(d.ranges, B * 8 + 64);
  a.take(d.index, B * cap * 4);
  a.take(d.outlier, B * cap);
  a.take(d.ninl, B * 4 + 64);
  a.take(d.ninl_first, B * 4 + 64);
  a.take(d.nobs_first, B * 4 + 64);
  a.take(d.ntracked, B * 4 + 64);
  a.take(d.status, B * 4 + 64);
  a.take(d.retry_nq, B * 4 + 64);
  a.take(d.foutl, B * cap + 64);
  a.take(d.store_err, 64);
  a.take(d.ref_kf, B * 4 + 64);
}

namespace {

// host [B][n][elem] -> device [B][stride][elem], zero padding behind n
int put_rows(vo_tracker *t, void *dst, const void *src, int n, int stride, size_t elem) {
  const size_t B = t->B;
  VO_HIP_CHECK(hipMemsetAsync(dst, 0, B * stride * elem, t->st));
  if (n > 0 && src)
    VO_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)stride * elem, src, (size_t)n * elem, (size_t)n * elem, B, hipMemcpyHostToDevice,
                                  t->st));
  return VO_OK;
}

struct StageTimer {
  vo_tracker *t;
  int stage;
  hipStream_t s;
  StageTimer(vo_tracker *t_, int stage_, hipStream_t s_) : t(t_), stage(stage_), s(s_) {
    if (t->tslot >= 0) (void)hipEventRecord(t->tev[(size_t)t->tslot * 2 * kStages + 2 * stage], s);
  }
  ~StageTimer() {
    if (t->tslot >= 0) (void)hipEventRecord(t->tev[(size_t)t->tslot * 2 * kStages + 2 * stage + 1], s);
  }
};

int collect_timing(vo_tracker *t) {
  if (t->tissued == 0) return VO_OK;
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  if (t->est != t->st) VO_HIP_CHECK(hipStreamSynchronize(t->est));
  for (int c = 0; c < t->tissued; c++) {
    for (int s = 0; s < kStages; s++) {
      float ms = 0.f;
      const size_t e = (size_t)c * 2 * kStages + 2 * s;
      if (hipEventElapsedTime(&ms, t->tev[e], t->tev[e + 1]) == hipSuccess) t->tms[s] += ms;
    }
    t->tcalls++;
  }
  t->tissued = 0;
  return VO_OK;
}

// the event set of the call about to be enqueued (created on first use)
int begin_timed_call(vo_tracker *t) {
  t->tslot = -1;
  if (!t->timing) return VO_OK;
  const size_t need = (size_t)(t->tissued + 1) * 2 * kStages;
  while (t->tev.size() < need) {
    hipEvent_t e;
    VO_HIP_CHECK(hipEventCreate(&e));
    t->tev.push_back(e);
  }
  t->tslot = t->tissued;
  return VO_OK;
}

int solve_pose(vo_tracker *t) {
  const vo_tracker::Arrays &d = t->d;
  if (t->pend.assigned) {
    VO_CHECK(vo_track_scatter_gather_dev(t->frames, 0, t->B, t->pend.assigned, t->pend.qpoints, t->pend.qflags, t->pend.stride,
                                         d.fpoint, d.fhas, d.fobs, t->sf, t->n_levels, d.pts, d.obs, d.isg, d.ranges, d.index, t->st));
    t->pend.assigned = nullptr;
  } else {
    VO_CHECK(vo_track_gather_dev(t->frames, 0, t->B, d.fpoint, d.fhas, t->sf, t->n_levels, d.pts, d.obs, d.isg, d.ranges, d.index,
                                 t->st));
  }
  return vo_pose_only_solve_ranges_dev(t->B, d.ranges, d.pts, d.obs, d.isg, d.Tcw + (size_t)t->B * 12, d.pose, d.outlier, d.ninl,
                                       nullptr, t->st);
}

// (what a call runs: the kRun* bits of tracker_state.h)

// the images and the depth of one call, in device memory (the host-buffer calls pass their uploaded copies)
struct FrameInput {
  const uint8_t *images;
  int img_pitch;
  size_t img_frame_stride;
  const void *depth;
  int depth_kind;  // 0 = none, 1 = float, 2 = uint16
  size_t depth_frame_stride;
  int depth_pitch;
};
// what every _dev entry point checks of its input
bool dev_input_ok(const vo_tracker *t, const FrameInput &in) {
  return t && in.images && in.img_pitch >= t->cfg.width && in.depth_kind >= 0 && in.depth_kind <= 2 && (!in.depth_kind || in.depth);
}

int stage_front(vo_tracker *t, const FrameInput &in, const void *host_depth) {
  const int B = t->B;
  hipStream_t st = t->st, est = t->est;
  const vo_tracker_config &c = t->cfg;
  // ---- extraction (its stream may be shared with other trackers)
  if (est != st && t->have_build) VO_HIP_CHECK(hipStreamWaitEvent(est, t->ev_build, 0));  // last batch's key-points consumed
  {
    StageTimer tm(t, 0, est);
    VO_CHECK(vo_orb_extract_batch_dev(t->orb, in.images, B, c.width, c.height, in.img_pitch, in.img_frame_stride, t->d.kps, t->d.desc,
                                      t->kcap, t->d.cnt));
  }
  VO_HIP_CHECK(hipEventRecord(t->ev_extract, est));
  if (est != st) VO_HIP_CHECK(hipStreamWaitEvent(st, t->ev_extract, 0));
  if (host_depth) {  // (see vo_tracker::cst)
    if (t->have_build) VO_HIP_CHECK(hipStreamWaitEvent(t->cst, t->ev_build, 0));  // the last call's depth has been consumed
    VO_HIP_CHECK(hipMemcpyAsync(t->depth.p, host_depth, t->pend_depth_bytes, hipMemcpyHostToDevice, t->cst));
    VO_HIP_CHECK(hipEventRecord(t->ev_depth, t->cst));
    VO_HIP_CHECK(hipStreamWaitEvent(st, t->ev_depth, 0));
  }
  // ---- Frame::Frame post-processing
  {
    StageTimer tm(t, 1, st);
    VO_CHECK(vo_frames_build_dev(t->frames, 0, B, t->d.kps, t->d.desc, t->d.cnt, t->kcap, in.depth, in.depth_kind,
                                 in.depth_frame_stride, in.depth_pitch, c.inv_depth_scale, st));
  }
  VO_HIP_CHECK(hipEventRecord(t->ev_build, st));
  t->have_build = true;
  return VO_OK;
}

// everything k_track_count / k_track_first_status / k_track_pack need to write the result block
PackArgs pack_args(vo_tracker *t) {
  t->have_result = true;
  return PackArgs{t->B, t->d.pose, t->d.ninl, t->d.nm_first, t->d.nm, vo::orb_error_flag(t->orb), vo::guided_error_flag(t->frames),
                  t->d.resblk, t->ref_store ? t->d.store_err : nullptr};
}
int launch_pack(vo_tracker *t) {
  hipLaunchKernelGGL(k_track_pack, dim3((t->B + 255) / 256), dim3(256), 0, t->st, pack_args(t), t->d.ntracked, t->d.status);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// trackWithMotion's search (visualOdometry.cpp:238-245): projection, searchByProjection(frame, last frame, radius), the
// retry at 2 x radius for frames with fewer than 20 matches, the map points of the matches into the frame's slots
int stage_motion(vo_tracker *t, const vo_tracker_params &P) {
  const int B = t->B;
  hipStream_t st = t->st;
  const vo_tracker_config &c = t->cfg;
  vo_guided_queries q{};
  vo_guided_params gp{};
  gp.n_levels = t->n_levels, gp.scale_factors = t->sf;
  StageTimer tm(t, 2, st);
  const vo_tracker::Arrays &d = t->d;
  const float cam4[4] = {c.intrinsics[0], c.intrinsics[1], c.intrinsics[2], c.intrinsics[3]};
  // (nq_last > 0 here: run_pipeline takes the first-frame route otherwise)
  hipLaunchKernelGGL(k_track_project_prep, dim3((t->nq_last + 255) / 256, B), dim3(256), 0, st, t->nq_last, t->n_last, d.Tcw, d.p0,
                     d.pf0, cam4[0], cam4[1], cam4[2], cam4[3], 0, c.width, 0, c.height, d.q0_flags, d.q0_u, d.q0_v, d.q0_aux, t->cap,
                     d.assigned, d.fhas, d.fobs, d.last_matched, d.pose0, d.pose);
  VO_HIP_CHECK(hipGetLastError());
  q.n_queries = t->nq_last, q.stride = t->n_last, q.flags = d.q0_flags, q.u = d.q0_u, q.v = d.q0_v, q.aux = d.q0_aux;
  q.level = d.q0_level, q.angle = d.q0_angle, q.desc = d.q0_desc;
  gp.mode = 0, gp.radius = P.radius, gp.bf = c.intrinsics[4], gp.direction = P.direction, gp.check_rot = 1;
  // `if (match_num < 20) { fill(mappoints_, nullptr); match_num = searchByProjection(..., 2*radius); }` (:241-245): the
  // first search's replay decides per frame (it knows the count), clears the assignments of the frames that need the
  // second look and writes their query counts; the second call leaves every other frame out (n_per_frame < 0) -- two
  // short dispatches (a candidate grid whose workgroups return at once, a replay) even when no frame needs them: ~8 us
  // per batch inside bench.py's `match_last_frame` stage
  if (!P.no_retry) gp.retry_below = 20, gp.retry_n_per_frame = d.retry_nq;
  VO_CHECK(vo_match_guided_dev(t->frames, 0, B, &q, &gp, nullptr, d.assigned, nullptr, d.nm_first, 0, st));
  if (!P.no_retry) {
    q.n_per_frame = d.retry_nq;
    gp.radius = 2.f * P.radius, gp.retry_n_per_frame = nullptr;
    VO_CHECK(vo_match_guided_dev(t->frames, 0, B, &q, &gp, nullptr, d.assigned, nullptr, d.nm_first, 0, st));
  }
  // the matches go into the frame's slots in the launch that gathers the pose problem (solve_pose)
  t->pend.assigned = d.assigned, t->pend.qpoints = d.p0, t->pend.qflags = d.q0_flags, t->pend.stride = t->n_last;
  return VO_OK;
}

// trackRefKeyFrame's search (visualOdometry.cpp:256-270): computeBow of the frames, searchByBoW(reference key-frame,
// frame) with Matcher(0.7); the key-frame's map points of the matches into the frame's slots, the pose starts at
// frame_last_->Tcw_ (vo_tracker_set_ref_keyframe).  The common-node walk is host work between two device steps
// (vo::bow_search_resident synchronises): this is the route of a frame that trackWithMotion has already given up on.
int stage_ref_keyframe(vo_tracker *t, const vo_tracker_params &P) {
  const int B = t->B;
  hipStream_t st = t->st;
  StageTimer tm(t, 2, st);
  if (!t->ref_vocab || (int)t->ref_kf.size() != B) {
    vo::set_error("vo_tracker_track_ref_keyframe: no reference key-frame (vo_tracker_set_ref_keyframe)");
    return VO_ERR_INVALID;
  }
  const vo_tracker::Arrays &d = t->d;
  hipLaunchKernelGGL(k_track_prep, dim3(B), dim3(256), 0, st, t->cap, t->n_last, d.assigned, d.fhas, d.fobs, d.last_matched, d.pose0,
                     d.pose);
  std::vector<vo::RefKeyFrame> kfs((size_t)B);
  for (int f = 0; f < B; f++) {
    const RefKfHost &k = t->ref_kf[f];
    kfs[f] = vo::RefKeyFrame{k.n, k.valid.data(), k.desc.data(), k.angle.data(), &k.view};
  }
  VO_CHECK(vo::bow_search_resident(t->ref_vocab, t->frames, 0, B, kfs.data(), P.ref_ratio > 0.f ? P.ref_ratio : 0.7f, 1, 3,
                                   d.assigned, t->cap, d.nm_first, st));
  // the matches go into the frame's slots in the launch that gathers the pose problem (solve_pose)
  t->pend.assigned = d.assigned, t->pend.qpoints = d.p0, t->pend.qflags = d.q0_flags, t->pend.stride = t->n_last;
  return VO_OK;
}

// The same search with the reference key-frames read from the key-frame store by number (vo_tracker_track_ref_keyframe_store):
// the frames' FeatureVectors (k_bow_transform, k_featvec), the key-frames' map points and the start pose out of the store
// (k_ref_kf_gather), the common-node walk on the device (k_bow_walk, one pair per frame, a bad key-frame searched like any
// other) and k_node_replay -- six launches, nothing but launches and two event operations around the store's stream.
int stage_ref_keyframe_store(vo_tracker *t, const vo_tracker_params &P) {
  const int B = t->B;
  hipStream_t st = t->st;
  StageTimer tm(t, 2, st);
  const vo_tracker::RefStoreArgs &A = *t->ref_store_args;
  const vo_tracker::Arrays &d = t->d;
  VO_CHECK(vo::bow_featvec_resident(A.vocab, t->frames, B, 3, t->walk, st));
  VO_CHECK(vo::kfstore_order_before(A.store, st));
  const vo::KfStoreView S = vo::kfstore_view(A.store);
  hipLaunchKernelGGL(k_ref_kf_gather, dim3((3 * t->n_last + 255) / 256, B), dim3(256), 0, st, S, A.ref_kf, A.Tcw12, t->n_last, d.p0,
                     d.pf0, d.q0_flags, d.Tcw, d.pose0, d.store_err);
  hipLaunchKernelGGL(k_track_prep, dim3(B), dim3(256), 0, st, t->cap, t->n_last, d.assigned, d.fhas, d.fobs, d.last_matched, d.pose0,
                     d.pose);
  VO_HIP_CHECK(hipGetLastError());
  // (the caller's numbers are free once the stream has passed this call: vo_tracker_build_local_map reads the copy)
  VO_HIP_CHECK(hipMemcpyAsync(d.ref_kf, A.ref_kf, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  VO_CHECK(vo::bow_walk_replay(t->frames, B, 1, S, A.ref_kf, P.ref_ratio > 0.f ? P.ref_ratio : 0.7f, 1, t->walk, d.assigned,
                               d.nm_first, st, nullptr, nullptr, true));
  VO_CHECK(vo::kfstore_order_after(A.store, st));
  t->pend.assigned = d.assigned, t->pend.qpoints = d.p0, t->pend.qflags = d.q0_flags, t->pend.stride = t->n_last;
  return VO_OK;
}

InFrameArgs in_frame_args(vo_tracker *t) {
  const vo_tracker_config &c = t->cfg;
  const vo_tracker::Arrays &d = t->d;
  return InFrameArgs{t->nq_local, t->n_local, d.pose, d.p1, d.nrm1, d.mind1, d.maxd1, d.pf1, t->have_link ? d.link1 : (const int *)nullptr,
                     d.last_matched, t->n_last, c.intrinsics[0], c.intrinsics[1], c.intrinsics[2], c.intrinsics[3], c.intrinsics[4], 0.f,
                     (float)c.width, 0.f, (float)c.height, (float)log((double)t->sf[1]), t->n_levels, d.q1_flags, d.q1_u, d.q1_v,
                     d.q1_aux, d.q1_level, d.q1_viewcos, nullptr};
}

// solvePoseOnlySE3 + cullingOutliersBeforeLocalMap (:249-250 / :271-272)
// (Round 5 tried the culling and the isInFrame pass of the local-map stage in ONE launch, one workgroup per frame with a barrier
//  between the two: 172 us per 1024 frames against 24 + 50 for the two launches -- a frame's ~1900 queries walked by 256 threads
//  in 8 dependent trips leave one wavefront per SIMD, where the separate kernel runs 8 workgroups per frame side by side.)
int stage_solve_cull(vo_tracker *t) {
  hipStream_t st = t->st;
  StageTimer tm(t, 3, st);
  VO_CHECK(solve_pose(t));
  const vo_tracker::Arrays &d = t->d;
  const CullArgs C{t->cap, d.ranges, d.index, d.outlier, d.assigned, t->n_last, d.fhas, d.fobs, d.last_matched, d.nobs_first,
                   d.assigned_first, d.pose, d.pose_first, d.ninl, d.ninl_first};
  hipLaunchKernelGGL(k_track_cull, dim3(t->B), dim3(256), 0, st, C);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

// trackLocalMap from searchLocalMapPoints on (:745-775, :289-300)
int stage_local(vo_tracker *t, const vo_tracker_params &P) {
  const int B = t->B;
  hipStream_t st = t->st;
  const vo_tracker_config &c = t->cfg;
  vo_guided_queries q{};
  vo_guided_params gp{};
  gp.n_levels = t->n_levels, gp.scale_factors = t->sf;
  const vo_tracker::Arrays &d = t->d;
  // ---- searchLocalMapPoints: isInFrame with the refined pose, then the search; occupied = holds an observed point
  {
    StageTimer tm(t, 4, st);
    if (t->nq_local > 0) {
      hipLaunchKernelGGL(k_track_in_frame, dim3((t->nq_local + 255) / 256, B), dim3(256), 0, st, in_frame_args(t));
      // (`assigned` was cleared by k_track_cull)
      q.n_queries = t->nq_local, q.stride = t->n_local, q.flags = d.q1_flags, q.u = d.q1_u, q.v = d.q1_v, q.aux = d.q1_aux;
      q.level = d.q1_level, q.viewcos = d.q1_viewcos, q.desc = d.q1_desc;
      gp.mode = 1, gp.radius = P.th_radius, gp.ratio = P.ratio, gp.bf = 0.f, gp.direction = 0, gp.check_rot = 0;
      VO_CHECK(vo_match_guided_dev(t->frames, 0, B, &q, &gp, d.fobs, d.assigned, nullptr, d.nm, 0, st));
      t->pend.assigned = d.assigned, t->pend.qpoints = d.p1, t->pend.qflags = d.q1_flags, t->pend.stride = t->n_local;
    } else {
      VO_HIP_CHECK(hipMemsetAsync(d.nm, 0, (size_t)B * 4, st));
    }
  }
  // ---- second solvePoseOnlySE3 and the inlier count of trackLocalMap
  {
    StageTimer tm(t, 5, st);
    VO_CHECK(solve_pose(t));
    hipLaunchKernelGGL(k_track_count, dim3(B), dim3(256), 0, st, t->cap, d.ranges, d.index, d.outlier, d.fobs, d.nm_first, d.nobs_first,
                       d.ninl_first, d.ntracked, d.status, t->first_min_matches, d.foutl, pack_args(t));
    VO_HIP_CHECK(hipGetLastError());
  }
  return VO_OK;
}

// VisualOdometry::relocalization() (:313-395) on the frames the front has built: reloc.hip works on the tracker's
// per-feature frame state and pose-solver buffers
vo::RelocShared reloc_shared(vo_tracker *t) {
  const vo_tracker_config &c = t->cfg;
  const vo_tracker::Arrays &d = t->d;
  vo::RelocShared S{};
  S.frames = t->frames, S.B = t->B, S.cap = t->cap, S.n_levels = t->n_levels, S.width = c.width, S.height = c.height, S.sf = t->sf;
  for (int i = 0; i < 5; i++) S.cam5[i] = c.intrinsics[i];
  S.cam5d = d.Tcw + (size_t)t->B * 12;
  S.pose = d.pose, S.fpoint = d.fpoint, S.fhas = d.fhas, S.foutl = d.foutl, S.fobs = d.fobs, S.pts = d.pts, S.obs = d.obs, S.isg = d.isg;
  S.ranges = d.ranges, S.index = d.index, S.outlier = d.outlier, S.ninl = d.ninl, S.assigned = d.assigned, S.nm = d.nm;
  S.resblk = d.resblk, S.orb_err = vo::orb_error_flag(t->orb), S.guided_err = vo::guided_error_flag(t->frames);
  S.st = t->st;
  return S;
}

// trackLocalMap behind a relocalisation (:61, :74, :82-83 -> :280-310): searchLocalMapPoints from the frame state the walk
// left in fpoint / fhas / fobs / foutl, the local points the frame already holds skipped by id, the search with
// occupied = the slot holds an observed point, the solve over all non-null slots, inliers_num_.  Frames whose
// relocalisation failed are left out of every launch.
int stage_local_reloc(vo_tracker *t, const vo_tracker_params &P) {
  const int B = t->B;
  hipStream_t st = t->st;
  const vo_tracker::Arrays &d = t->d;
  const vo::RelocShared S = reloc_shared(t);
  const vo::RelocLocalArgs L{t->nq_local, t->n_local, d.pf1, d.q1_flags, t->have_ids ? d.ids1 : (const int *)nullptr, d.p1};
  const int *frame_on = nullptr;
  VO_CHECK(vo::reloc_local_prep(t->reloc, S, L, &frame_on));
  if (t->nq_local > 0) {
    InFrameArgs A = in_frame_args(t);
    A.pflags = d.q1_flags, A.link = nullptr, A.frame_on = frame_on;  // (a thread reads its point's flags before it writes them)
    hipLaunchKernelGGL(k_track_in_frame, dim3((t->nq_local + 255) / 256, B), dim3(256), 0, st, A);
    VO_HIP_CHECK(hipGetLastError());
    vo_guided_queries q{};
    vo_guided_params gp{};
    gp.n_levels = t->n_levels, gp.scale_factors = t->sf;
    q.n_queries = t->nq_local, q.stride = t->n_local, q.n_per_frame = frame_on, q.flags = d.q1_flags, q.u = d.q1_u, q.v = d.q1_v;
    q.aux = d.q1_aux, q.level = d.q1_level, q.viewcos = d.q1_viewcos, q.desc = d.q1_desc;
    gp.mode = 1, gp.radius = P.th_radius, gp.ratio = P.ratio, gp.bf = 0.f, gp.direction = 0, gp.check_rot = 0;
    VO_CHECK(vo_match_guided_dev(t->frames, 0, B, &q, &gp, d.fobs, d.assigned, nullptr, d.nm, 0, st));
  } else {
    VO_HIP_CHECK(hipMemsetAsync(d.nm, 0, (size_t)B * 4, st));
  }
  return vo::reloc_local_finish(t->reloc, S, L);
}

int stage_reloc(vo_tracker *t) {
  const vo::RelocShared S = reloc_shared(t);
  t->have_result = true;
  if (!t->store_args) return vo::reloc_run(t->reloc, S);
  vo::RelocStoreArgs A = *t->store_args;
  t->rtimed = false;
  if (t->timing) {  // events around the four new stages of the call (vo_tracker_get_reloc_timing)
    for (hipEvent_t &e : t->rtev)
      if (!e) VO_HIP_CHECK(hipEventCreate(&e));
    A.tev = t->rtev;
  }
  VO_CHECK(vo::reloc_run_store(t->reloc, S, A));
  t->rtimed = t->timing;
  return VO_OK;
}

int run_pipeline(vo_tracker *t, const FrameInput &in, const vo_tracker_params *prm, unsigned run) {
  // (the host depth image of THIS call, if any: taken off the handle before anything can fail, so that a call that ends early never
  //  leaves a host pointer behind for the next one)
  const void *host_depth = t->pend_depth;
  t->pend_depth = nullptr;
  VO_CHECK(begin_timed_call(t));
  t->pend.assigned = nullptr;  // (a call that failed half-way must not leave its matches to the next one)
  if (!(run == (kRunFront | kRunMotion | kRunLocal))) t->tslot = -1;  // the six stage timers describe the one-call tracked frame
  const int B = t->B;
  hipStream_t st = t->st;
  vo_tracker_params P;
  if (prm) {
    P = *prm;
  } else {
    P.radius = 15.f, P.th_radius = 3.f, P.ratio = 0.8f, P.direction = 0, P.no_retry = 0, P.ref_ratio = 0.7f;
  }
  if (run & kRunFront) {
    t->ref_store = (run & kRunRefStore) != 0;
    t->last_reloc = (run & kRunReloc) != 0;
    t->ids_route = ((run & kRunReloc) && t->store_args) ? 1 : ((run & kRunRefStore) && !(run & kRunLocal)) ? 2 : 0;
    VO_CHECK(stage_front(t, in, host_depth));
  }
  if (run & kRunReloc) return stage_reloc(t);
  const size_t capB = (size_t)B * t->cap;
  if ((run & kRunMotion) && t->nq_last == 0) {
    // no last frame (the first frame of a sequence, visualOdometry.cpp:170-214): Frame construction only; the pose is
    // the one handed in, every count zero
    VO_HIP_CHECK(hipMemcpyAsync(t->d.pose, t->d.pose0, (size_t)B * 48, hipMemcpyDeviceToDevice, st));
    VO_HIP_CHECK(hipMemcpyAsync(t->d.pose_first, t->d.pose0, (size_t)B * 48, hipMemcpyDeviceToDevice, st));
    VO_HIP_CHECK(hipMemsetAsync(t->d.assigned, 0xff, capB * 4, st));
    VO_HIP_CHECK(hipMemsetAsync(t->d.assigned_first, 0xff, capB * 4, st));
    VO_HIP_CHECK(hipMemsetAsync(t->d.fhas, 0, capB, st));
    for (int *count : {t->d.nm, t->d.nm_first, t->d.ninl, t->d.ninl_first, t->d.nobs_first, t->d.ntracked, t->d.status})
      VO_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)B * 4, st));
    VO_CHECK(launch_pack(t));
    t->tslot = -1;  // Frame construction only: not a timed tracked frame
    return VO_OK;
  }
  if (run & kRunMotion) {
    t->first_min_matches = 20;  // :247
    VO_CHECK(stage_motion(t, P));
  } else if (run & kRunRefKeyFrame) {
    t->first_min_matches = 15;  // :268
    VO_CHECK(stage_ref_keyframe(t, P));
  } else if (run & kRunRefStore) {
    t->first_min_matches = 15;  // :268
    VO_CHECK(stage_ref_keyframe_store(t, P));
  }
  if (run & (kRunMotion | kRunRefKeyFrame | kRunRefStore)) VO_CHECK(stage_solve_cull(t));
  // (the result block is written by the last kernel of either route: k_track_count / k_track_first_status)
  if (run & kRunLocal) {
    VO_CHECK(stage_local(t, P));
  } else {
    // first stage only: the status word and the counts of trackWithMotion / trackRefKeyFrame
    VO_HIP_CHECK(hipMemsetAsync(t->d.nm, 0, (size_t)B * 4, st));
    hipLaunchKernelGGL(k_track_first_status, dim3((B + 255) / 256), dim3(256), 0, st, B, t->d.nm_first, t->d.nobs_first, t->d.ntracked,
                       t->d.status, t->first_min_matches, pack_args(t));
    VO_HIP_CHECK(hipGetLastError());
  }
  if (t->tslot >= 0) t->tissued++, t->tslot = -1;
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_tracker_create(vo_tracker **out, const vo_tracker_config *cfg) {
  if (!out || !cfg || cfg->batch < 1 || cfg->width < 64 || cfg->height < 64 || cfg->max_last < 1 || cfg->max_local < 0)
    return VO_ERR_INVALID;
  VO_CHECK(vo::ensure_device());
  vo_tracker *t = new (std::nothrow) vo_tracker();
  if (!t) {
    vo::set_error("vo_tracker_create: out of host memory");
    return VO_ERR_HIP;
  }
  t->cfg = *cfg;
  t->B = cfg->batch;
  int rc = vo_orb_create(&t->orb, cfg->nfeatures > 0 ? cfg->nfeatures : 1000, cfg->scale_factor > 1.f ? cfg->scale_factor : 1.2f,
                         cfg->nlevels > 0 ? cfg->nlevels : 8, cfg->ini_th_fast > 0 ? cfg->ini_th_fast : 20,
                         cfg->min_th_fast > 0 ? cfg->min_th_fast : 7);
  if (rc != VO_OK) {
    delete t;
    return rc;
  }
  auto fail = [&](int code) {
    vo_tracker_destroy(t);
    return code;
  };
  if (cfg->stream) {
    t->st = (hipStream_t)cfg->stream;
  } else {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(&t->st, hipStreamNonBlocking, hi) != hipSuccess) return fail(VO_ERR_HIP);
    t->own_st = true;
  }
  if (cfg->extract_stream) {
    t->est = (hipStream_t)cfg->extract_stream;
  } else if (cfg->single_stream) {
    t->est = t->st;
  } else {
    if (hipStreamCreateWithFlags(&t->est, hipStreamNonBlocking) != hipSuccess) return fail(VO_ERR_HIP);
    t->own_est = true;
  }
  if ((rc = vo_orb_set_stream(t->orb, t->est)) != VO_OK) return fail(rc);
  if (hipEventCreateWithFlags(&t->ev_extract, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&t->ev_build, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&t->ev_depth, hipEventDisableTiming) != hipSuccess ||
      hipStreamCreateWithFlags(&t->cst, hipStreamNonBlocking) != hipSuccess)
    return fail(VO_ERR_HIP);
  t->n_levels = vo_orb_levels(t->orb);
  if ((rc = vo_orb_scale_factors(t->orb, t->sf, nullptr)) != VO_OK) return fail(rc);
  t->kcap = vo_orb_max_keypoints(t->orb);
  t->cap = cfg->max_features > 0 ? cfg->max_features : std::max(256, (t->kcap + 63) / 64 * 64);
  t->n_last = cfg->max_last, t->n_local = std::max(cfg->max_local, 1);
  if ((rc = vo_frames_create(&t->frames, t->B, t->cap)) != VO_OK) return fail(rc);
  if ((rc = vo_frames_set_camera(t->frames, cfg->intrinsics, cfg->has_distortion ? cfg->dist_coef : nullptr, (float)cfg->width,
                                 (float)cfg->height)) != VO_OK)
    return fail(rc);
  if ((rc = t->mem.build([&](vo::Arena &a) { t->layout(a); }, "vo_tracker_create")) != VO_OK) return fail(rc);
  // rows that no route writes for a frame it leaves out (a failed relocalisation) read as zero in every tracker, whatever
  // the allocator handed back
  if (hipMemset(t->mem.block, 0, t->mem.bytes ? t->mem.bytes : 4096) != hipSuccess) return fail(VO_ERR_HIP);
  if ((rc = t->kps.reserve((size_t)t->B * t->kcap * sizeof(vo_keypoint))) != VO_OK || (rc = t->desc.reserve((size_t)t->B * t->kcap * 32)) != VO_OK)
    return fail(rc);
  t->d.kps = t->kps.as<vo_keypoint>(), t->d.desc = t->desc.as<uint8_t>();
  if (hipMemset(t->d.store_err, 0, 64) != hipSuccess) return fail(VO_ERR_HIP);
  if (cfg->max_reloc_candidates > 0 || cfg->max_reloc_features > 0) {
    if (cfg->max_reloc_candidates < 1 || cfg->max_reloc_candidates > 256 || cfg->max_reloc_features < 1) return fail(VO_ERR_INVALID);
    if ((rc = vo::reloc_create(&t->reloc, t->B, t->cap, cfg->max_reloc_candidates, cfg->max_reloc_features, t->sf, t->n_levels)) != VO_OK)
      return fail(rc);
  }
  // the intrinsics as doubles behind the Tcw block (the pose solver reads them from device memory)
  {
    double cam5d[5];
    for (int i = 0; i < 5; i++) cam5d[i] = (double)cfg->intrinsics[i];
    if (hipMemcpy(t->d.Tcw + (size_t)t->B * 12, cam5d, sizeof(cam5d), hipMemcpyHostToDevice) != hipSuccess) return fail(VO_ERR_HIP);
  }
  *out = t;
  return VO_OK;
}

void vo_tracker_destroy(vo_tracker *t) {
  if (!t) return;
  if (t->st) (void)hipStreamSynchronize(t->st);
  if (t->est && t->est != t->st) (void)hipStreamSynchronize(t->est);
  if (t->cst) (void)hipStreamSynchronize(t->cst);
  for (hipEvent_t e : t->tev)
    if (e) (void)hipEventDestroy(e);
  if (t->ev_extract) (void)hipEventDestroy(t->ev_extract);
  if (t->ev_build) (void)hipEventDestroy(t->ev_build);
  if (t->ev_depth) (void)hipEventDestroy(t->ev_depth);
  if (t->reloc) vo::reloc_destroy(t->reloc);
  vo::handover_destroy(t->ho);
  vo::motion_store_destroy(t->ms);
  for (hipEvent_t e : t->rtev)
    if (e) (void)hipEventDestroy(e);
  if (t->frames) vo_frames_destroy(t->frames);
  if (t->orb) vo_orb_destroy(t->orb);
  if (t->own_st && t->st) (void)hipStreamDestroy(t->st);
  if (t->own_est && t->est) (void)hipStreamDestroy(t->est);
  if (t->cst) (void)hipStreamDestroy(t->cst);
  delete t;
}

int vo_tracker_info(const vo_tracker *t, int *batch, int *max_features, int *max_keypoints, int *n_levels) {
  if (!t) return VO_ERR_INVALID;
  if (batch) *batch = t->B;
  if (max_features) *max_features = t->cap;
  if (max_keypoints) *max_keypoints = t->kcap;
  if (n_levels) *n_levels = t->n_levels;
  return VO_OK;
}

vo_orb *vo_tracker_extractor(vo_tracker *t) { return t ? t->orb : nullptr; }
vo_frames *vo_tracker_frames(vo_tracker *t) { return t ? t->frames : nullptr; }
void *vo_tracker_stream(vo_tracker *t) { return t ? (void *)t->st : nullptr; }

int vo_tracker_set_last_frame(vo_tracker *t, int n, const double *Tcw12, const double *points, const uint8_t *flags,
                              const int32_t *octave, const float *angle, const uint8_t *desc) {
  if (!t || n < 0 || n > t->n_last || !Tcw12 || (n > 0 && (!points || !flags || !octave || !angle || !desc)))
    return VO_ERR_INVALID;
  const int B = t->B;
  // pose6 = log(Tcw) on the host (the solver's start value; Frame::setPose keeps the SE3 itself)
  std::vector<double> p6((size_t)B * 6);
  for (int f = 0; f < B; f++) VO_CHECK(vo_se3_log(Tcw12 + 12 * f, Tcw12 + 12 * f + 9, p6.data() + 6 * f));
  VO_CHECK(t->stage.reserve((size_t)B * 144));
  memcpy(t->stage.data(), Tcw12, (size_t)B * 96);
  memcpy(t->stage.data() + (size_t)B * 96, p6.data(), (size_t)B * 48);
  VO_HIP_CHECK(hipMemcpyAsync(t->d.Tcw, t->stage.data(), (size_t)B * 96, hipMemcpyHostToDevice, t->st));
  VO_HIP_CHECK(hipMemcpyAsync(t->d.pose0, t->stage.data() + (size_t)B * 96, (size_t)B * 48, hipMemcpyHostToDevice, t->st));
  VO_CHECK(put_rows(t, t->d.p0, points, n, t->n_last, 24));
  VO_CHECK(put_rows(t, t->d.pf0, flags, n, t->n_last, 1));
  VO_CHECK(put_rows(t, t->d.q0_level, octave, n, t->n_last, 4));
  VO_CHECK(put_rows(t, t->d.q0_angle, angle, n, t->n_last, 4));
  VO_CHECK(put_rows(t, t->d.q0_desc, desc, n, t->n_last, 32));
  t->nq_last = n;
  t->have_last_ids = false, t->handed_over = false;  // (ids belong to the list they were set for)
  VO_HIP_CHECK(hipStreamSynchronize(t->st));  // the caller's arrays and the staging block are free again
  return VO_OK;
}

int vo_tracker_set_local_map(vo_tracker *t, int n, const double *points, const double *normals, const float *min_distance,
                             const float *max_distance, const uint8_t *flags, const int32_t *link, const uint8_t *desc) {
  if (!t || n < 0 || n > t->n_local || (n > 0 && (!points || !normals || !min_distance || !max_distance || !flags || !desc)))
    return VO_ERR_INVALID;
  VO_CHECK(put_rows(t, t->d.p1, points, n, t->n_local, 24));
  VO_CHECK(put_rows(t, t->d.nrm1, normals, n, t->n_local, 24));
  VO_CHECK(put_rows(t, t->d.mind1, min_distance, n, t->n_local, 4));
  VO_CHECK(put_rows(t, t->d.maxd1, max_distance, n, t->n_local, 4));
  VO_CHECK(put_rows(t, t->d.pf1, flags, n, t->n_local, 1));
  VO_CHECK(put_rows(t, t->d.q1_desc, desc, n, t->n_local, 32));
  t->have_link = link != nullptr;
  if (link) VO_CHECK(put_rows(t, t->d.link1, link, n, t->n_local, 4));
  t->nq_local = n;
  t->have_local = true, t->have_ids = false;  // (ids belong to the local map they were set for)
  t->lm_route = 0, t->local_ran = false;      // (a host-set map: vo_tracker_end_frame_store is refused)
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  return VO_OK;
}

int vo_tracker_set_local_map_ids(vo_tracker *t, int n, const int32_t *ids) {
  if (!t) return VO_ERR_INVALID;
  if (!t->have_local || n != t->nq_local || (n > 0 && !ids)) {
    vo::set_error("vo_tracker_set_local_map_ids: %d ids for a local map of %d points (vo_tracker_set_local_map first)", n,
                  t->have_local ? t->nq_local : -1);
    return VO_ERR_INVALID;
  }
  VO_CHECK(put_rows(t, t->d.ids1, ids, n, t->n_local, 4));
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  t->have_ids = true;
  t->lm_route = 0;  // (ids of the caller's, not the store's)
  return VO_OK;
}

// what vo_tracker_end_frame asks of the last track call: the stages it ran, all of them enqueued
static int ran(vo_tracker *t, unsigned run, int rc) {
  t->last_run = rc == VO_OK ? run : 0u;
  t->handed_over = false;  // (the frame store's slots hold another frame now)
  t->lm_motion = false, t->local_split = false;
  t->lm_route = 0, t->local_ran = false;
  return rc;
}

static int track_dev(vo_tracker *t, const FrameInput &in, const vo_tracker_params *params, unsigned run) {
  if (!dev_input_ok(t, in)) return VO_ERR_INVALID;
  return ran(t, run, run_pipeline(t, in, params, run));
}

int vo_tracker_track_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                         const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                         const vo_tracker_params *params) {
  return track_dev(t, {dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch}, params,
                   kRunFront | kRunMotion | kRunLocal);
}

static int upload_host_frames(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind, size_t *npx_out, size_t *dsz_out) {
  const size_t B = t->B, npx = (size_t)t->cfg.width * t->cfg.height, dsz = depth_kind == 1 ? 4 : depth_kind == 2 ? 2 : 0;
  VO_CHECK(t->images.reserve(B * npx));
  if (dsz) VO_CHECK(t->depth.reserve(B * npx * dsz));
  // uploads on the extraction stream (the depth is first read behind the extraction, which the tracking stream waits for)
  if (t->est != t->st && t->have_build) VO_HIP_CHECK(hipStreamWaitEvent(t->est, t->ev_build, 0));
  VO_HIP_CHECK(hipMemcpyAsync(t->images.p, images, B * npx, hipMemcpyHostToDevice, t->est));
  // (the depth follows behind the extraction's launches, on the copy stream: stage_front)
  t->pend_depth = dsz ? depth : nullptr, t->pend_depth_bytes = B * npx * dsz;
  *npx_out = npx, *dsz_out = dsz;
  return VO_OK;
}

static int track_host(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind, const vo_tracker_params *params,
                      unsigned run) {
  if (!t || !images || depth_kind < 0 || depth_kind > 2 || (depth_kind && !depth)) return VO_ERR_INVALID;
  size_t npx = 0, dsz = 0;
  VO_CHECK(upload_host_frames(t, images, depth, depth_kind, &npx, &dsz));
  const FrameInput in{t->images.as<uint8_t>(), t->cfg.width, npx, dsz ? t->depth.p : nullptr, depth_kind, npx * dsz, t->cfg.width * (int)dsz};
  return ran(t, run, run_pipeline(t, in, params, run));
}

int vo_tracker_track_first(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind, const vo_tracker_params *params) {
  return track_host(t, images, depth, depth_kind, params, kRunFront | kRunMotion);
}

int vo_tracker_track_first_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                               const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                               const vo_tracker_params *params) {
  return track_dev(t, {dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch}, params,
                   kRunFront | kRunMotion);
}

int vo_tracker_track_local_map(vo_tracker *t, const vo_tracker_params *params) {
  if (!t) return VO_ERR_INVALID;
  if (!t->have_result) {
    vo::set_error("vo_tracker_track_local_map: no first stage has run (vo_tracker_track_first / _ref_keyframe_first)");
    return VO_ERR_INVALID;
  }
  if (t->last_reloc) {  // behind vo_tracker_relocalize*: the hand-over (checked before anything is enqueued)
    if (!t->have_local) {
      vo::set_error("vo_tracker_track_local_map: no local map has been set (vo_tracker_set_local_map)");
      return VO_ERR_INVALID;
    }
    vo_tracker_params P;
    if (params) P = *params;
    else P.radius = 15.f, P.th_radius = 5.f, P.ratio = 0.8f, P.direction = 0, P.no_retry = 0, P.ref_ratio = 0.7f;  // :768
    t->pend.assigned = nullptr;
    const int rc = stage_local_reloc(t, P);
    t->local_ran = rc == VO_OK;
    return rc;
  }
  const int rc = run_pipeline(t, FrameInput{}, params, kRunLocal);
  t->last_run = rc == VO_OK ? (t->last_run | kRunLocal) : 0u;
  t->local_split = rc == VO_OK, t->local_ran = rc == VO_OK;
  return rc;
}

int vo_tracker_track_ref_keyframe(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind,
                                  const vo_tracker_params *params, int first_stage_only) {
  return track_host(t, images, depth, depth_kind, params, kRunFront | kRunRefKeyFrame | (first_stage_only ? 0u : kRunLocal));
}

int vo_tracker_track_ref_keyframe_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                                      const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                                      const vo_tracker_params *params, int first_stage_only) {
  return track_dev(t, {dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch}, params,
                   kRunFront | kRunRefKeyFrame | (first_stage_only ? 0u : kRunLocal));
}

int vo_tracker_set_ref_keyframe(vo_tracker *t, const vo_vocab *vocab, int n, const double *Tcw12, const double *points,
                                const uint8_t *flags, const float *angle, const uint8_t *desc, const vo_bow_view *const *nodes) {
  if (!t || !vocab || n < 0 || n > t->n_last || !Tcw12 || !nodes || (n > 0 && (!points || !flags || !angle || !desc)))
    return VO_ERR_INVALID;
  const int B = t->B;
  // every view is validated BEFORE anything is enqueued or any tracker state changes: a DBoW3::FeatureVector as CSR
  // has start[0] == 0, non-decreasing offsets, every feature index below n; an empty view may carry null arrays
  for (int f = 0; f < B; f++) {
    const vo_bow_view *v = nodes[f];
    if (!v || v->n_nodes < 0 || (v->n_nodes > 0 && (!v->node_id || !v->start || !v->feat))) {
      vo::set_error("vo_tracker_set_ref_keyframe: frame %d has no usable vocabulary-node view", f);
      return VO_ERR_INVALID;
    }
    if (v->n_nodes == 0) continue;
    if (v->start[0] != 0) {
      vo::set_error("vo_tracker_set_ref_keyframe: frame %d: start[0] = %d", f, v->start[0]);
      return VO_ERR_INVALID;
    }
    for (int j = 0; j < v->n_nodes; j++)
      if (v->start[j + 1] < v->start[j]) {
        vo::set_error("vo_tracker_set_ref_keyframe: frame %d: node offsets decrease at node %d", f, j);
        return VO_ERR_INVALID;
      }
    const int nf = v->start[v->n_nodes];
    for (int i = 0; i < nf; i++)
      if ((int)v->feat[i] < 0 || (int)v->feat[i] >= n) {
        vo::set_error("vo_tracker_set_ref_keyframe: frame %d names feature %u of %d", f, v->feat[i], n);
        return VO_ERR_INVALID;
      }
  }
  std::vector<double> p6((size_t)B * 6);
  for (int f = 0; f < B; f++) VO_CHECK(vo_se3_log(Tcw12 + 12 * f, Tcw12 + 12 * f + 9, p6.data() + 6 * f));
  VO_CHECK(t->stage.reserve((size_t)B * 144));
  memcpy(t->stage.data(), Tcw12, (size_t)B * 96);
  memcpy(t->stage.data() + (size_t)B * 96, p6.data(), (size_t)B * 48);
  VO_HIP_CHECK(hipMemcpyAsync(t->d.Tcw, t->stage.data(), (size_t)B * 96, hipMemcpyHostToDevice, t->st));
  VO_HIP_CHECK(hipMemcpyAsync(t->d.pose0, t->stage.data() + (size_t)B * 96, (size_t)B * 48, hipMemcpyHostToDevice, t->st));
  // the key-frame's map points take the place of the last frame's list: the tail of the pipeline (scatter, culling, the
  // `link` test of the local-map stage) indexes them exactly as it indexes frame_last_->mappoints_
  VO_CHECK(put_rows(t, t->d.p0, points, n, t->n_last, 24));
  VO_CHECK(put_rows(t, t->d.pf0, flags, n, t->n_last, 1));
  VO_CHECK(put_rows(t, t->d.q0_flags, flags, n, t->n_last, 1));
  std::vector<RefKfHost> kfs((size_t)B);
  for (int f = 0; f < B; f++) {
    RefKfHost &k = kfs[f];
    const vo_bow_view *v = nodes[f];
    k.n = n;
    k.valid.resize((size_t)n), k.angle.assign(angle + (size_t)f * n, angle + (size_t)(f + 1) * n);
    for (int i = 0; i < n; i++) k.valid[i] = flags[(size_t)f * n + i] & 1;
    k.desc.assign(desc + (size_t)f * n * 32, desc + (size_t)(f + 1) * n * 32);
    if (v->n_nodes > 0) {
      k.node_id.assign(v->node_id, v->node_id + v->n_nodes);
      k.start.assign(v->start, v->start + v->n_nodes + 1);
      k.feat.assign(v->feat, v->feat + v->start[v->n_nodes]);
    } else {
      k.start.assign(1, 0);
    }
    k.view.n_nodes = v->n_nodes, k.view.node_id = reinterpret_cast<const uint32_t *>(k.node_id.data()), k.view.start = k.start.data(),
    k.view.feat = k.feat.data();
  }
  VO_HIP_CHECK(hipStreamSynchronize(t->st));  // (the staging block may be reused by the next call)
  t->ref_vocab = vocab;  // only now: a call that failed above leaves the tracker's reference key-frame as it was
  t->ref_kf.swap(kfs);
  // the views point into the vectors' heap blocks, which the swap moved along with their owners
  t->nq_last = n;
  t->have_last_ids = false, t->handed_over = false;
  return VO_OK;
}

// The BoW walk buffers of the store routes, sized from the tracker's capacities: max_reloc_candidates key-frames per frame
// (trackRefKeyFrame: one) of up to `nk` features, nk = the bound of the calling route on a store's max_features
// (relocalisation: max_reloc_features, trackRefKeyFrame: max_last).  The buffers only ever grow, and only on the first call
// of a route that needs more than the routes used so far: a tracker that never runs trackRefKeyFrame from the store keeps
// the relocalisation footprint it had.
static int walk_reserve(vo_tracker *t, int nk) {
  if (t->walk.B != 0 && nk > t->walk.NK) VO_HIP_CHECK(hipStreamSynchronize(t->st));  // (growing frees the block an enqueued route may still read)
  return vo::bow_walk_reserve(t->walk, t->B, t->cap, std::max(t->cfg.max_reloc_candidates, 1), std::max(nk, t->walk.NK), t->st);
}

// what the store form of trackRefKeyFrame checks before anything is enqueued; sizes the walk buffers on the first call
static int ref_store_ready(vo_tracker *t, const char *call, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_ref_kf,
                           const double *dev_Tcw12) {
  if (!t) return VO_ERR_INVALID;
  if (!store || !vocab || !dev_ref_kf || !dev_Tcw12) {
    vo::set_error("%s: no store, no vocabulary, or no key-frame numbers / poses", call);
    return VO_ERR_INVALID;
  }
  const vo::KfStoreView V = vo::kfstore_view(store);
  if (V.NK > t->n_last) {
    vo::set_error("%s: the store holds %d features per key-frame, the tracker %d (max_last)", call, V.NK, t->n_last);
    return VO_ERR_CAPACITY;
  }
  return walk_reserve(t, t->n_last);
}

// only behind a call that was enqueued (as vo_tracker_set_ref_keyframe commits "only now"): like that call the route
// replaces the last-frame state, and the host route's reference key-frame is gone
static void ref_store_commit(vo_tracker *t, const char *call, const vo_kfstore *store) {
  t->store_call = call;
  t->ref_vocab = nullptr, t->ref_kf.clear();
  // the rows hold max_features entries, flag 0 beyond a key-frame's own n (which only the device knows): a following
  // vo_tracker_track without vo_tracker_set_last_frame would project those dead queries too
  t->nq_last = vo::kfstore_view(store).NK;
  t->have_last_ids = false, t->handed_over = false;
}

int vo_tracker_track_ref_keyframe_store(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_ref_kf,
                                        const double *dev_Tcw12, const uint8_t *images, const void *depth, int depth_kind,
                                        const vo_tracker_params *params, int first_stage_only) {
  if (!t || !images || depth_kind < 0 || depth_kind > 2 || (depth_kind && !depth)) return VO_ERR_INVALID;
  VO_CHECK(ref_store_ready(t, "vo_tracker_track_ref_keyframe_store", store, vocab, dev_ref_kf, dev_Tcw12));
  const vo_tracker::RefStoreArgs A{store, vocab, dev_ref_kf, dev_Tcw12};
  t->ref_store_args = &A;
  const int rc = track_host(t, images, depth, depth_kind, params, kRunFront | kRunRefStore | (first_stage_only ? 0u : kRunLocal));
  t->ref_store_args = nullptr;
  if (rc == VO_OK) ref_store_commit(t, "vo_tracker_track_ref_keyframe_store", store);
  return rc;
}

int vo_tracker_track_ref_keyframe_store_dev(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_ref_kf,
                                            const double *dev_Tcw12, const uint8_t *dev_images, int image_pitch,
                                            size_t image_frame_stride, const void *dev_depth, int depth_kind,
                                            size_t depth_frame_stride, int depth_pitch, const vo_tracker_params *params,
                                            int first_stage_only) {
  const FrameInput in{dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch};
  if (!dev_input_ok(t, in)) return VO_ERR_INVALID;
  VO_CHECK(ref_store_ready(t, "vo_tracker_track_ref_keyframe_store_dev", store, vocab, dev_ref_kf, dev_Tcw12));
  const vo_tracker::RefStoreArgs A{store, vocab, dev_ref_kf, dev_Tcw12};
  t->ref_store_args = &A;
  const int rc = track_dev(t, in, params, kRunFront | kRunRefStore | (first_stage_only ? 0u : kRunLocal));
  t->ref_store_args = nullptr;
  if (rc == VO_OK) ref_store_commit(t, "vo_tracker_track_ref_keyframe_store_dev", store);
  return rc;
}

static int reloc_ready(vo_tracker *t) {
  if (!t) return VO_ERR_INVALID;
  if (!t->reloc) {
    vo::set_error("vo_tracker: the relocalisation route is not configured (vo_tracker_config.max_reloc_candidates / _features)");
    return VO_ERR_INVALID;
  }
  return VO_OK;
}

int vo_tracker_set_reloc_candidates(vo_tracker *t, const vo_vocab *vocab, int max_cand, const int32_t *n_cand,
                                    const vo_reloc_candidate *cands) {
  VO_CHECK(reloc_ready(t));
  return vo::reloc_set_candidates(t->reloc, vocab, max_cand, n_cand, cands, t->st);
}

int vo_tracker_relocalize(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind, const vo_tracker_params *params) {
  VO_CHECK(reloc_ready(t));
  return track_host(t, images, depth, depth_kind, params, kRunFront | kRunReloc);
}

int vo_tracker_relocalize_dev(vo_tracker *t, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                              const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                              const vo_tracker_params *params) {
  VO_CHECK(reloc_ready(t));
  return track_dev(t, {dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch}, params,
                   kRunFront | kRunReloc);
}

// what both store routes check before anything is enqueued; sizes the route's buffers on the first call
static int store_route_ready(vo_tracker *t, const char *call, vo_kfdb *db, const vo_kfstore *store, const vo_vocab *vocab) {
  VO_CHECK(reloc_ready(t));
  if (!store || !vocab) {
    vo::set_error("%s: no store or no vocabulary", call);
    return VO_ERR_INVALID;
  }
  const vo::KfStoreView V = vo::kfstore_view(store);
  if (V.NK > t->cfg.max_reloc_features) {
    vo::set_error("%s: the store holds %d features per key-frame, the tracker %d (max_reloc_features)", call, V.NK,
                  t->cfg.max_reloc_features);
    return VO_ERR_CAPACITY;
  }
  if (db) {
    int size = 0, max_batch = 0;
    vo::kfdb_info(db, &size, &max_batch);
    if (size != V.size) {
      vo::set_error("%s: the database holds %d key-frames, the store %d", call, size, V.size);
      return VO_ERR_INVALID;
    }
    if (max_batch < t->B) {
      vo::set_error("%s: a batch of %d frames, the database was created for batches of %d", call, t->B, max_batch);
      return VO_ERR_CAPACITY;
    }
  }
  VO_CHECK(walk_reserve(t, t->cfg.max_reloc_features));
  t->store_call = call;
  return vo::reloc_store_prepare(t->reloc, &t->walk, t->d.store_err, db != nullptr, t->st);
}

static int store_route_host(vo_tracker *t, const vo::RelocStoreArgs &A, const uint8_t *images, const void *depth, int depth_kind,
                            const vo_tracker_params *params) {
  t->store_args = &A;
  const int rc = track_host(t, images, depth, depth_kind, params, kRunFront | kRunReloc);
  t->store_args = nullptr;
  return rc;
}

static int store_route_dev(vo_tracker *t, const vo::RelocStoreArgs &A, const FrameInput &in, const vo_tracker_params *params) {
  t->store_args = &A;
  const int rc = track_dev(t, in, params, kRunFront | kRunReloc);
  t->store_args = nullptr;
  return rc;
}

int vo_tracker_relocalize_store(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_n_cand,
                                const int32_t *dev_cand, int cand_stride, const uint8_t *images, const void *depth, int depth_kind,
                                const vo_tracker_params *params) {
  VO_CHECK(store_route_ready(t, "vo_tracker_relocalize_store", nullptr, store, vocab));
  if (!dev_n_cand || !dev_cand || cand_stride < 1) return VO_ERR_INVALID;
  const vo::RelocStoreArgs A{store, vocab, dev_n_cand, dev_cand, cand_stride, nullptr, nullptr, nullptr};
  return store_route_host(t, A, images, depth, depth_kind, params);
}

int vo_tracker_relocalize_store_dev(vo_tracker *t, const vo_kfstore *store, const vo_vocab *vocab, const int32_t *dev_n_cand,
                                    const int32_t *dev_cand, int cand_stride, const uint8_t *dev_images, int image_pitch,
                                    size_t image_frame_stride, const void *dev_depth, int depth_kind, size_t depth_frame_stride,
                                    int depth_pitch, const vo_tracker_params *params) {
  VO_CHECK(store_route_ready(t, "vo_tracker_relocalize_store_dev", nullptr, store, vocab));
  if (!dev_n_cand || !dev_cand || cand_stride < 1) return VO_ERR_INVALID;
  const vo::RelocStoreArgs A{store, vocab, dev_n_cand, dev_cand, cand_stride, nullptr, nullptr, nullptr};
  return store_route_dev(t, A, {dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch}, params);
}

int vo_tracker_relocalize_db(vo_tracker *t, vo_kfdb *db, const vo_kfstore *store, const vo_vocab *vocab, const float *dev_stale_score,
                             const uint8_t *images, const void *depth, int depth_kind, const vo_tracker_params *params) {
  if (!db) return VO_ERR_INVALID;
  VO_CHECK(store_route_ready(t, "vo_tracker_relocalize_db", db, store, vocab));
  const vo::RelocStoreArgs A{store, vocab, nullptr, nullptr, 0, db, dev_stale_score, nullptr};
  return store_route_host(t, A, images, depth, depth_kind, params);
}

int vo_tracker_relocalize_db_dev(vo_tracker *t, vo_kfdb *db, const vo_kfstore *store, const vo_vocab *vocab,
                                 const float *dev_stale_score, const uint8_t *dev_images, int image_pitch, size_t image_frame_stride,
                                 const void *dev_depth, int depth_kind, size_t depth_frame_stride, int depth_pitch,
                                 const vo_tracker_params *params) {
  if (!db) return VO_ERR_INVALID;
  VO_CHECK(store_route_ready(t, "vo_tracker_relocalize_db_dev", db, store, vocab));
  const vo::RelocStoreArgs A{store, vocab, nullptr, nullptr, 0, db, dev_stale_score, nullptr};
  return store_route_dev(t, A, {dev_images, image_pitch, image_frame_stride, dev_depth, depth_kind, depth_frame_stride, depth_pitch}, params);
}

int vo_tracker_build_local_map(vo_tracker *t, vo_kfstore *store) {
  if (!t || !store) return VO_ERR_INVALID;
  // everything is checked before anything is enqueued
  // the motion route: the first stage alone has run, and the last-frame list it searched carries ids (section 4v)
  const bool motion = t->have_result && t->ids_route == 0 && t->last_run == (kRunFront | kRunMotion) && t->have_last_ids;
  if (!t->have_result || (t->ids_route == 0 && !motion)) {
    vo::set_error("vo_tracker_build_local_map: the last route left no map-point ids (valid after vo_tracker_relocalize_store / _db, "
                  "vo_tracker_track_ref_keyframe_store with first_stage_only = 1, and vo_tracker_track_first with ids on the "
                  "last-frame list)");
    return VO_ERR_INVALID;
  }
  if (t->cfg.max_local < 1) {
    vo::set_error("vo_tracker_build_local_map: the tracker holds no local points (max_local = 0)");
    return VO_ERR_INVALID;
  }
  const vo::KfStoreView V = vo::kfstore_view(store);
  if (t->ids_route == 2 && V.NK > t->n_last) {
    vo::set_error("vo_tracker_build_local_map: the store holds %d features per key-frame, the tracker %d (max_last)", V.NK, t->n_last);
    return VO_ERR_CAPACITY;
  }
  int *fid = nullptr;
  const int *winner = nullptr;
  if (t->ids_route == 1) VO_CHECK(vo::reloc_frame_ids(t->reloc, &fid, &winner));
  if (motion) VO_CHECK(vo::motion_store_ensure(t));
  hipStream_t st = t->st;
  if (V.max_kf > t->lm_max_kf) {  // the first call, or a store of more key-frames than any before
    if (t->lm_max_kf) VO_HIP_CHECK(hipStreamSynchronize(st));  // (growing frees the block an enqueued call may still use)
    const size_t B = t->B;
    t->lm = {};
    t->lm_max_kf = 0;
    VO_CHECK(t->lm_mem.build(
        [&](vo::Arena &a) {
          a.take(t->lm.votes, B * (size_t)V.max_kf * 4);
          a.take(t->lm.lkf, B * VO_TRACKER_LOCAL_MAX_KEYFRAMES * 4);
          a.take(t->lm.n_kf, B * 4 + 64);
          a.take(t->lm.best, B * 4 + 64);
          a.take(t->lm.n_pts, B * 4 + 64);
        },
        "vo_tracker_build_local_map"));
    t->lm_max_kf = V.max_kf;
  }
  vo::LocalMapArgs A{};
  VO_CHECK(vo::kfstore_obs_view(store, &A.O));  // (rebuilds the observation index on the store's stream when it is stale)
  VO_CHECK(vo::kfstore_order_before(store, st));
  const vo_tracker::Arrays &d = t->d;
  A.S = vo::kfstore_view(store);
  A.B = t->B, A.cap = t->cap, A.max_local = t->cfg.max_local, A.stride = t->n_local;
  A.fn = vo::frame_store_view(t->frames).n;
  A.winner = winner, A.sid = fid;
  if (t->ids_route == 2) A.ref_kf = d.ref_kf, A.assigned = d.assigned_first;
  A.fhas = d.fhas, A.fobs = d.fobs;
  A.votes = t->lm.votes, A.lkf = t->lm.lkf, A.n_kf = t->lm.n_kf, A.best = t->lm.best, A.n_pts = t->lm.n_pts;
  A.err = d.store_err;
  A.p1 = d.p1, A.nrm1 = d.nrm1, A.mind1 = d.mind1, A.maxd1 = d.maxd1, A.pf1 = d.pf1, A.desc1 = d.q1_desc, A.link1 = d.link1, A.ids1 = d.ids1;
  if (motion) VO_CHECK(vo::motion_store_slot_ids(t, &A, st));  // (the ids gathered from the last list: A.sid and its vote mask)
  VO_CHECK(vo::local_map_build(A, st));
  if (motion) VO_CHECK(vo::motion_store_link(t, st));
  // the sticky word into the result block (its third flag), as the store routes leave it
  VO_HIP_CHECK(hipMemcpyAsync(d.resblk + (size_t)t->B * 72 + 8, d.store_err, 4, hipMemcpyDeviceToDevice, st));
  VO_CHECK(vo::kfstore_order_after(store, st));
  t->nq_local = t->cfg.max_local;
  t->have_local = true, t->have_ids = true, t->have_link = t->ids_route == 2 || motion;
  t->lm_motion = motion;
  t->lm_route = motion ? 0 : t->ids_route, t->local_ran = false;  // (vo_tracker_end_frame_store: this frame's map, no local stage yet)
  return VO_OK;
}

int vo_tracker_get_reloc_timing(vo_tracker *t, double *ms) {
  if (!t || !ms) return VO_ERR_INVALID;
  if (!t->rtimed) {
    vo::set_error("vo_tracker_get_reloc_timing: no store route has run with timing on (vo_tracker_set_timing)");
    return VO_ERR_INVALID;
  }
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  for (int s = 0; s < VO_TRACKER_RELOC_STAGES; s++) {
    float v = 0.f;
    VO_HIP_CHECK(hipEventElapsedTime(&v, t->rtev[2 * s], t->rtev[2 * s + 1]));
    ms[s] = v;
  }
  return VO_OK;
}

int vo_tracker_track(vo_tracker *t, const uint8_t *images, const void *depth, int depth_kind, const vo_tracker_params *params) {
  return track_host(t, images, depth, depth_kind, params, kRunFront | kRunMotion | kRunLocal);
}

int vo_tracker_results(vo_tracker *t, double *poses6, double *Tcw12, int32_t *n_tracked, int32_t *n_inliers,
                       int32_t *n_matches_last, int32_t *n_matches_local, int32_t *status) {
  if (!t) return VO_ERR_INVALID;
  const size_t B = t->B;
  if (!t->have_result) {  // nothing has been tracked yet
    vo::set_error("vo_tracker_results: no batch has been tracked");
    return VO_ERR_INVALID;
  }
  VO_CHECK(t->stage.reserve(B * 72 + 64));
  uint8_t *h = t->stage.data();
  VO_HIP_CHECK(hipMemcpyAsync(h, t->d.resblk, B * 72 + 12, hipMemcpyDeviceToHost, t->st));  // one download: k_track_pack's block
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  int32_t *dst[5] = {n_tracked, n_inliers, n_matches_last, n_matches_local, status};
  for (size_t f = 0; f < B; f++) {
    const double *p6 = reinterpret_cast<const double *>(h + f * 72);
    const int32_t *pi = reinterpret_cast<const int32_t *>(h + f * 72 + 48);
    if (poses6) memcpy(poses6 + 6 * f, p6, 48);
    if (Tcw12) VO_CHECK(vo_se3_exp(p6, Tcw12 + 12 * f, Tcw12 + 12 * f + 9));
    for (int k = 0; k < 5; k++)
      if (dst[k]) dst[k][f] = pi[k];
  }
  const int32_t *flags = reinterpret_cast<const int32_t *>(h + B * 72);
  // (the third word is the store routes' only -- and the motion route's once vo_tracker_build_local_map has run behind it)
  const int32_t store_err = (t->ref_store || t->lm_motion || vo::reloc_last_was_store(t->reloc)) ? flags[2] : 0;
  if (flags[0] != 0 || flags[1] != 0) {
    // a sticky error flag of a stage is up (dropped key-points, exhausted candidate pools): report and clear it
    VO_CHECK(vo_orb_sync(t->orb));
    VO_CHECK(vo_match_guided_status(t->frames, t->st));
  }
  if (store_err) {  // report and clear
    VO_HIP_CHECK(hipMemsetAsync(t->d.store_err, 0, 4, t->st));
    VO_HIP_CHECK(hipMemsetAsync(t->d.resblk + B * 72 + 8, 0, 4, t->st));
    if (store_err & 2) {
      vo::set_error("%s: a key-frame number lies outside the store (treated as a key-frame without features)", t->store_call);
      return VO_ERR_INVALID;
    }
    if (store_err & (vo::kStoreErrLocalPoints | vo::kStoreErrLocalKfs)) {
      vo::set_error("vo_tracker_build_local_map: a frame has more distinct local points than max_local = %d, or more voting key-frames "
                    "than %d; the first of them in order were kept (VO_TRACKER_LOCAL_N_POINTS / _N_KEYFRAMES hold the true counts)",
                    t->cfg.max_local, VO_TRACKER_LOCAL_MAX_KEYFRAMES);
      return VO_ERR_CAPACITY;
    }
    vo::set_error("%s: a frame has more candidates than the tracker walks (max_reloc_candidates = %d); the first %d were walked",
                  t->store_call, t->cfg.max_reloc_candidates, t->cfg.max_reloc_candidates);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

int vo_tracker_get(vo_tracker *t, int what, void *dst, size_t dst_bytes) {
  if (!t || !dst) return VO_ERR_INVALID;
  const size_t B = t->B, cap = t->cap;
  const void *b = nullptr;
  size_t bytes = 0;
  if (what >= VO_TRACKER_RELOC_WINNER && what <= VO_TRACKER_RELOC_N_CANDIDATES) {
    VO_CHECK(reloc_ready(t));
    const void *src = vo::reloc_selector(t->reloc, what, &bytes);
    if (!src) {
      if (what >= VO_TRACKER_RELOC_CANDIDATES)
        vo::set_error("vo_tracker_get(%d): the last route was not vo_tracker_relocalize_store / _db", what);
      return VO_ERR_INVALID;
    }
    if (dst_bytes < bytes) {
      vo::set_error("vo_tracker_get(%d): destination holds %zu bytes, %zu needed", what, dst_bytes, bytes);
      return VO_ERR_CAPACITY;
    }
    VO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, t->st));
    VO_HIP_CHECK(hipStreamSynchronize(t->st));
    return VO_OK;
  }
  if (what == VO_TRACKER_LAST_N) {  // (a host value: the last-frame list's n)
    if (dst_bytes < 4) return VO_ERR_CAPACITY;
    const int32_t n = t->nq_last;
    memcpy(dst, &n, 4);
    return VO_OK;
  }
  switch (what) {
    case VO_TRACKER_ASSIGNED_LAST: b = t->d.assigned_first, bytes = B * cap * 4; break;
    case VO_TRACKER_ASSIGNED_LOCAL: b = t->d.assigned, bytes = B * cap * 4; break;
    case VO_TRACKER_POSE_FIRST: b = t->d.pose_first, bytes = B * 48; break;
    case VO_TRACKER_INLIERS_FIRST: b = t->d.ninl_first, bytes = B * 4; break;
    case VO_TRACKER_OBSERVED_INLIERS_FIRST: b = t->d.nobs_first, bytes = B * 4; break;
    case VO_TRACKER_FEATURE_HAS_POINT: b = t->d.fhas, bytes = B * cap; break;
    case VO_TRACKER_FEATURE_POINTS: b = t->d.fpoint, bytes = B * cap * 24; break;
    case VO_TRACKER_LOCAL_FLAGS: b = t->d.q1_flags, bytes = B * (size_t)t->n_local; break;
    case VO_TRACKER_LOCAL_U: b = t->d.q1_u, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_V: b = t->d.q1_v, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_UR: b = t->d.q1_aux, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_LEVEL: b = t->d.q1_level, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_VIEWCOS: b = t->d.q1_viewcos, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_KEYPOINT_COUNTS: b = t->d.cnt, bytes = B * 4; break;
    case VO_TRACKER_FEATURE_OUTLIER: b = t->d.foutl, bytes = B * cap; break;
    case VO_TRACKER_LOCAL_KEYFRAMES: b = t->lm.lkf, bytes = B * VO_TRACKER_LOCAL_MAX_KEYFRAMES * 4; break;
    case VO_TRACKER_LOCAL_N_KEYFRAMES: b = t->lm.n_kf, bytes = B * 4; break;
    case VO_TRACKER_LOCAL_N_POINTS: b = t->lm.n_pts, bytes = B * 4; break;
    case VO_TRACKER_LOCAL_REF_KF: b = t->lm.best, bytes = B * 4; break;
    case VO_TRACKER_LOCAL_POINT_IDS: b = t->d.ids1, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_POINTS: b = t->d.p1, bytes = B * (size_t)t->n_local * 24; break;
    case VO_TRACKER_LOCAL_NORMALS: b = t->d.nrm1, bytes = B * (size_t)t->n_local * 24; break;
    case VO_TRACKER_LOCAL_MIN_DISTANCE: b = t->d.mind1, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_MAX_DISTANCE: b = t->d.maxd1, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_LOCAL_DESC: b = t->d.q1_desc, bytes = B * (size_t)t->n_local * 32; break;
    case VO_TRACKER_LOCAL_MAP_FLAGS: b = t->d.pf1, bytes = B * (size_t)t->n_local; break;
    case VO_TRACKER_LOCAL_LINK: b = t->d.link1, bytes = B * (size_t)t->n_local * 4; break;
    case VO_TRACKER_POSE_START: b = t->d.pose0, bytes = B * 48; break;
    case VO_TRACKER_LAST_POINTS: b = t->d.p0, bytes = B * (size_t)t->n_last * 24; break;
    case VO_TRACKER_LAST_FLAGS: b = t->d.pf0, bytes = B * (size_t)t->n_last; break;
    case VO_TRACKER_LAST_OCTAVE: b = t->d.q0_level, bytes = B * (size_t)t->n_last * 4; break;
    case VO_TRACKER_LAST_ANGLE: b = t->d.q0_angle, bytes = B * (size_t)t->n_last * 4; break;
    case VO_TRACKER_LAST_DESC: b = t->d.q0_desc, bytes = B * (size_t)t->n_last * 32; break;
    case VO_TRACKER_TCW_START: b = t->d.Tcw, bytes = B * 96; break;
    case VO_TRACKER_FEATURE_OBSERVED: b = t->d.fobs, bytes = B * cap; break;
    default:
      if (what < VO_TRACKER_SLOT_IDS || what > VO_TRACKER_REF_KF) return VO_ERR_INVALID;
      b = what >= VO_TRACKER_FIRST_SLOT_IDS ? vo::motion_store_selector(t, what, &bytes)  // (the block of motion_store.hip)
                                            : vo::handover_selector(t, what, &bytes);     // (the block of handover.hip)
  }
  if (!b) {
    vo::set_error("vo_tracker_get(%d): %s has not run", what,
                  what >= VO_TRACKER_FIRST_SLOT_IDS ? "the motion route from the store (vo_tracker_build_local_map after vo_tracker_track_first, "
                                                      "vo_tracker_point_stats[_arrays], vo_tracker_record_ref_pose)"
                  : what >= VO_TRACKER_SLOT_IDS     ? "the hand-over (vo_tracker_end_frame, _set_last_pose, _set_last_frame_ids)"
                                                    : "vo_tracker_build_local_map");
    return VO_ERR_INVALID;
  }
  if (dst_bytes < bytes) {
    vo::set_error("vo_tracker_get(%d): destination holds %zu bytes, %zu needed", what, dst_bytes, bytes);
    return VO_ERR_CAPACITY;
  }
  VO_HIP_CHECK(hipMemcpyAsync(dst, b, bytes, hipMemcpyDeviceToHost, t->st));
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  return VO_OK;
}

int vo_frames_construct(vo_frames *h, int slot, vo_orb *orb, const uint8_t *image, int width, int height, int stride,
                        const void *depth, int depth_kind, int depth_pitch_bytes, float inv_depth_scale,
                        vo_keypoint *keypoints, int capacity, int *n_keypoints) {
  if (!h || !orb || !image || width < 1 || height < 1 || stride < width || depth_kind < 0 || depth_kind > 2 ||
      (depth_kind && (!depth || depth_pitch_bytes < width * (depth_kind == 1 ? 4 : 2))) || !n_keypoints || capacity < 0)
    return VO_ERR_INVALID;
  VO_CHECK(vo::ensure_device());
  hipStream_t st = vo::thread_stream();
  thread_local vo::ScratchBuf d_img, d_dep, d_kp, d_desc, d_cnt;
  thread_local vo::PinnedBuf stage;
  const int kcap = vo_orb_max_keypoints(orb);
  const size_t img_bytes = (size_t)stride * height, dep_bytes = depth_kind ? (size_t)depth_pitch_bytes * height : 0;
  VO_CHECK(d_img.reserve(img_bytes));
  VO_CHECK(d_dep.reserve(std::max<size_t>(dep_bytes, 64)));
  VO_CHECK(d_kp.reserve((size_t)kcap * sizeof(vo_keypoint)));
  VO_CHECK(d_desc.reserve((size_t)kcap * 32));
  VO_CHECK(d_cnt.reserve(64));
  VO_CHECK(vo_orb_set_stream(orb, st));
  VO_CHECK(vo::copy_h2d(d_img.p, image, img_bytes, st, "vo_frames_construct"));
  if (dep_bytes) VO_CHECK(vo::copy_h2d(d_dep.p, depth, dep_bytes, st, "vo_frames_construct"));
  VO_CHECK(vo_orb_extract_batch_dev(orb, d_img.as<uint8_t>(), 1, width, height, stride, img_bytes, d_kp.as<vo_keypoint>(),
                                    d_desc.as<uint8_t>(), kcap, d_cnt.as<int32_t>()));
  VO_CHECK(vo_frames_build_dev(h, slot, 1, d_kp.as<vo_keypoint>(), d_desc.as<uint8_t>(), d_cnt.as<int32_t>(), kcap,
                               dep_bytes ? d_dep.p : nullptr, depth_kind, dep_bytes, depth_pitch_bytes, inv_depth_scale, st));
  VO_CHECK(stage.reserve((size_t)kcap * sizeof(vo_keypoint) + 64));
  VO_CHECK(vo::copy_d2h(stage.data(), d_cnt.p, 4, st, "vo_frames_construct"));
  VO_CHECK(vo::copy_d2h(stage.data() + 64, d_kp.p, (size_t)kcap * sizeof(vo_keypoint), st, "vo_frames_construct"));
  VO_CHECK(vo::stream_sync(st, "vo_frames_construct"));
  VO_CHECK(vo_orb_sync(orb));
  int n = 0;
  memcpy(&n, stage.data(), 4);
  if (n > capacity) {
    vo::set_error("vo_frames_construct: %d key-points, capacity %d", n, capacity);
    return VO_ERR_CAPACITY;
  }
  if (keypoints && n > 0) memcpy(keypoints, stage.data() + 64, (size_t)n * sizeof(vo_keypoint));
  *n_keypoints = n;
  return VO_OK;
}

int vo_tracker_sync(vo_tracker *t) {
  if (!t) return VO_ERR_INVALID;
  VO_HIP_CHECK(hipStreamSynchronize(t->st));
  return VO_OK;
}

int vo_tracker_set_timing(vo_tracker *t, int enabled) {
  if (!t) return VO_ERR_INVALID;
  VO_CHECK(collect_timing(t));  // (synchronises only if timed calls are outstanding)
  t->timing = enabled != 0;
  t->tissued = 0, t->tslot = -1;
  for (double &m : t->tms) m = 0;
  t->tcalls = 0;
  return VO_OK;
}

int vo_tracker_get_timing(vo_tracker *t, double *ms, int *n_calls) {
  if (!t || !ms) return VO_ERR_INVALID;
  VO_CHECK(collect_timing(t));
  for (int s = 0; s < kStages; s++) ms[s] = t->tms[s], t->tms[s] = 0;
  if (n_calls) *n_calls = t->tcalls;
  t->tcalls = 0;
  return VO_OK;
}

}  // extern "C"
