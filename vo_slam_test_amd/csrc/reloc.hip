// reloc.hip -- the relocalisation route of the tracker (vo_tracker_relocalize): VisualOdometry::relocalization()
// (reference src/visualOdometry.cpp:313-395) for a batch of frames resident in the tracker's frame store, the ordered
// walk over every frame's candidate key-frames sequenced on the device.
//
//   independent front, one pass over all B x MC (frame, candidate) pairs
//     searchByBoW(kf, frame), Matcher(0.75)         vo::bow_search_resident (k_bow_transform, host node walk, k_node_replay)
//     poseEstimateByPnP's correspondence lists      k_reloc_count + k_reloc_scan + k_reloc_gather (ragged, device offsets)
//     solvePnPRansac(100, 8.0, 0.99, EPNP)          vo_pnp_ransac_dev
//   dependent tail, MC rounds enqueued unconditionally; round r = candidate r of every frame still walking
//     the PnP inliers and pose into the frame       k_reloc_apply (+ the gather of the first solve)
//     solvePoseOnlySE3                              k_pose_only                                  (x 3)
//     the gates of :342-387, culling                k_reloc_after_solve                          (x 3)
//     searchByProjection(frame, kf, r, th, found)   k_reloc_project + vo_match_guided_dev mode 2 (x 2)
//     its matches into the frame, the `>= 50` gate  k_reloc_after_search (+ the gather of the next solve)
//   k_reloc_finish: status word, result block
//
// A frame that does not take part in a step has a negative count in that step's per-frame array: its workgroups return
// at once.  All of a frame's walk state is one 8-int record (kRec*) that one workgroup per frame reads and rewrites.
#include "kfstore.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "ba_math.h"
#include "block_sort.h"

namespace {

using namespace vo;
using namespace vo::ba;

enum { kRecStage = 0, kRecDone = 1, kRecInliers = 2, kRecWinner = 3, kRecInts = 8 };
enum { kIdle = 0, kSolve1 = 1, kTop1 = 2, kSolve2 = 3, kTop2 = 4, kSolve3 = 5 };
enum { kOutBad = 0, kOutFewBow = 1, kOutFewPnp = 2, kOutFewSolve = 3, kOutBelow50 = 4, kOutSuccess = 5, kOutNotReached = 6 };

struct RelocDev {
  int B, cap, MC, NK;  // frames, feature slots per frame, candidates per frame, features per candidate (capacities)
  // frame store
  const int *fn;
  const float *X, *Y, *UR;
  const int *OCT;
  float *sf;
  // candidates [B * MC][NK]
  const int *n_cand;      // [B]
  int *kf_n;              // [B * MC]
  uint8_t *kf_bad;        // [B * MC]
  uint8_t *kf_flags;
  double *kf_point;
  int *kf_id;
  float *kf_mind, *kf_maxd;
  // front
  int *bow_assigned;  // [B * MC][cap]
  int *bow_n;         // [B * MC]
  int *cnt, *off;           // [B * MC], [B * MC + 1]
  float *p3, *p2;
  int *src;
  double *pnp_T;
  uint8_t *pnp_mask;
  int *pnp_n, *pnp_status;
  uint8_t *dbg_mask;  // [B * MC][cap]
  // walk state
  int *rec;            // [B][kRecInts]
  int *fid;            // [B][cap]
  uint8_t *found;      // [B][MC * NK] by id
  int *out_bow, *out_pnp, *out_code;  // [B][MC]
  int *nq;             // [B] per-frame query count of the guided search
  uint8_t *qflags;     // [B * MC][NK]
  float *qu, *qv;
  int *qlevel;
  int *ninl_solve;     // [B] the solver's return value (0 for frames left out)
  // the tracker's
  double *pose, *fpoint;
  uint8_t *fhas, *foutl;
  uint8_t *fobs;  // [B][cap] the slot's map point has observations (bit 1 of the source feature's flags): the `occupied` of the
                  // local-map search behind a relocalisation (matcher.cpp:314)
  double *pts, *obs, *isg;
  int *ranges, *index;
  const uint8_t *outlier;
  int *assigned;
  const int *nm;
};

// block-wide sum of one int per thread (256 threads)
__device__ __forceinline__ int block_sum(int v, int *s4) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return s4[0] + s4[1] + s4[2] + s4[3];
}

// poseEstimateByPnP's loop over mappointsMatches (:784-799): how many correspondences pair p contributes.  A pair that
// is absent, bad or below 15 matches is a zero-length problem.
__global__ __launch_bounds__(256) void k_reloc_count(RelocDev D) {
  __shared__ int s4[4];
  const int p = blockIdx.x, f = p / D.MC, c = p % D.MC;
  const int n = min(D.fn[f], D.cap);
  int local = 0;
  for (int i = threadIdx.x; i < n; i += 256) local += D.bow_assigned[(size_t)p * D.cap + i] >= 0;
  const int total = block_sum(local, s4);
  if (threadIdx.x == 0) {
    const bool live = c < D.n_cand[f] && !D.kf_bad[p] && D.bow_n[p] >= 15;
    D.cnt[p] = live ? total : 0;
  }
}

// exclusive prefix sum of the P counts: one workgroup, every thread a run of consecutive pairs
__global__ __launch_bounds__(256) void k_reloc_scan(int P, const int *cnt, int *off) {
  __shared__ int s_sum[256];
  const int tid = threadIdx.x, per = (P + 255) / 256, b = tid * per, e = min(b + per, P);
  int s = 0;
  for (int i = b; i < e; i++) s += cnt[i];
  s_sum[tid] = s;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; t++) base += s_sum[t];
  for (int i = b; i < e; i++) off[i] = base, base += cnt[i];
  if (tid == 255) off[P] = base;
}

// the correspondences of pair p in feature order (the lane mapping of k_track_gather): pts3d = the matched key-frame
// feature's map point as float, pts2d = unKeypoints_[i].pt, src = i
__global__ __launch_bounds__(256) void k_reloc_gather(RelocDev D) {
  __shared__ int wsum[4];
  __shared__ int s_base;
  const int p = blockIdx.x, f = p / D.MC, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int o0 = D.off[p], m = D.off[p + 1] - o0;
  if (m <= 0) return;
  const int n = min(D.fn[f], D.cap);
  const size_t fo = (size_t)f * D.cap, po = (size_t)p * D.cap, ko = (size_t)p * D.NK;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int b = 0; b < n; b += 256) {
    const int i = b + tid;
    const int a = i < n ? D.bow_assigned[po + i] : -1;
    const bool has = a >= 0;
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(has);
    const int within = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
    if (lane == 0) wsum[wave] = __popcll(mk);
    __syncthreads();
    int pre = s_base;
    for (int w = 0; w < wave; w++) pre += wsum[w];
    const int pos = pre + within;
    if (has && pos < m) {
      const size_t d = (size_t)o0 + pos;
      const double *P3 = D.kf_point + 3 * (ko + a);
      D.p3[3 * d] = (float)P3[0], D.p3[3 * d + 1] = (float)P3[1], D.p3[3 * d + 2] = (float)P3[2];  // cv::Point3f(pos) :794
      D.p2[2 * d] = D.X[fo + i], D.p2[2 * d + 1] = D.Y[fo + i];
      D.src[d] = i;
    }
    __syncthreads();
    if (tid == 0) s_base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// debug view of the PnP problems per frame feature (VO_TRACKER_RELOC_PNP_MASK)
__global__ __launch_bounds__(256) void k_reloc_pnp_mask(RelocDev D) {
  const int p = blockIdx.x;
  const size_t po = (size_t)p * D.cap;
  for (int i = threadIdx.x; i < D.cap; i += 256) D.dbg_mask[po + i] = 0;
  __syncthreads();
  const int o0 = D.off[p], m = D.off[p + 1] - o0;
  for (int j = threadIdx.x; j < m; j += 256) D.dbg_mask[po + D.src[o0 + j]] = (uint8_t)(1 + (D.pnp_mask[o0 + j] != 0));
}

// optimizer_ceres.cpp:181-202 over the frame's (id, position) slots: the features that hold a map point, in feature
// order, into the pose solver's observation list (k_track_gather's arithmetic and lane mapping).  Called by all 256
// threads of the frame's workgroup.
__device__ __forceinline__ void gather_frame(const RelocDev &D, int f, int *wsum, int *s_base) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(D.fn[f], D.cap);
  const size_t o = (size_t)f * D.cap;
  if (tid == 0) *s_base = 0;
  __syncthreads();
  for (int b = 0; b < n; b += 256) {
    const int i = b + tid;
    const bool has = i < n && D.fhas[o + i];
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(has);
    const int within = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
    if (lane == 0) wsum[wave] = __popcll(mk);
    __syncthreads();
    int pre = *s_base;
    for (int w = 0; w < wave; w++) pre += wsum[w];
    if (has) {
      const size_t d = o + pre + within;
      D.pts[3 * d] = D.fpoint[3 * (o + i)], D.pts[3 * d + 1] = D.fpoint[3 * (o + i) + 1], D.pts[3 * d + 2] = D.fpoint[3 * (o + i) + 2];
      D.obs[3 * d] = (double)D.X[o + i], D.obs[3 * d + 1] = (double)D.Y[o + i], D.obs[3 * d + 2] = (double)D.UR[o + i];
      D.isg[d] = 1.0 / (double)D.sf[D.OCT[o + i]];  // :190
      D.index[d] = i;
    }
    __syncthreads();
    if (tid == 0) *s_base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) D.ranges[2 * f] = (int)o, D.ranges[2 * f + 1] = *s_base;
}

// Round r, first step: candidate r of frame f.  The gates that need nothing of the walk (:323, :330), then
// poseEstimateByPnP's write-back (:808-825): the inliers' map points into the frame's slots and the pose into the frame
// BEFORE the count is tested at :336 -- a candidate with 1..9 inliers is rejected with both left behind.  A candidate
// that passes leaves found = its inliers' ids and the observation list of the first solve.
__global__ __launch_bounds__(256) void k_reloc_apply(RelocDev D, int r) {
  __shared__ int wsum[4];
  __shared__ int s_base, s_go;
  const int f = blockIdx.x, tid = threadIdx.x;
  int *rec = D.rec + (size_t)f * kRecInts;
  const size_t o = (size_t)f * D.cap;
  if (r == 0) {  // a freshly constructed frame (visualOdometry.cpp:57-63): every slot null, outliers_ clear
    for (int i = tid; i < D.cap; i += 256) D.fid[o + i] = -1, D.fhas[o + i] = 0, D.foutl[o + i] = 0, D.fobs[o + i] = 0;
    if (tid < 6) D.pose[6 * f + tid] = 0.0;
    if (tid < D.MC) D.out_code[f * D.MC + tid] = kOutNotReached, D.out_bow[f * D.MC + tid] = 0, D.out_pnp[f * D.MC + tid] = 0;
  }
  const bool done = r == 0 ? false : rec[kRecDone] != 0;
  __syncthreads();
  const int p = f * D.MC + r;
  int stage = kIdle;
  if (!done && r < D.n_cand[f]) {
    const int nbow = D.kf_bad[p] ? 0 : D.bow_n[p];
    const int npnp = (D.kf_bad[p] || nbow < 15 || D.pnp_status[p] != 1) ? 0 : D.pnp_n[p];
    int code;
    if (D.kf_bad[p]) code = kOutBad;
    else if (nbow < 15) code = kOutFewBow;
    else code = kOutFewPnp;
    if (npnp > 0) {
      const int o0 = D.off[p], m = D.off[p + 1] - o0;
      const size_t ko = (size_t)p * D.NK;
      const bool pass = npnp >= 10;
      uint8_t *found = D.found + (size_t)f * D.MC * D.NK;
      if (pass) {
        for (int i = tid; i < D.MC * D.NK; i += 256) found[i] = 0;
        __syncthreads();
      }
      for (int j = tid; j < m; j += 256) {
        if (!D.pnp_mask[o0 + j]) continue;
        const int i = D.src[o0 + j], a = D.bow_assigned[(size_t)p * D.cap + i];
        const double *P3 = D.kf_point + 3 * (ko + a);
        D.fpoint[3 * (o + i)] = P3[0], D.fpoint[3 * (o + i) + 1] = P3[1], D.fpoint[3 * (o + i) + 2] = P3[2];
        D.fhas[o + i] = 1, D.fobs[o + i] = (D.kf_flags[ko + a] >> 1) & 1u;
        const int id = D.kf_id[ko + a];
        D.fid[o + i] = id;
        if (pass) found[id] = 1;
      }
      if (tid == 0) {  // cv::Rodrigues(r, R); poseRtToSE3; frame->setPose (:820-823)
        const double *T = D.pnp_T + 12 * (size_t)p;
        const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
        double xi[6];
        se3_log_from_R(R, t, xi);
        for (int k = 0; k < 6; k++) D.pose[6 * f + k] = xi[k];
      }
      if (pass) stage = kSolve1;
    }
    if (tid == 0) {
      D.out_bow[p] = nbow, D.out_pnp[p] = npnp;
      if (stage == kIdle) D.out_code[p] = code;
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (r == 0) rec[kRecDone] = 0, rec[kRecInliers] = 0, rec[kRecWinner] = -1;
    rec[kRecStage] = stage;
    if (stage == kIdle) D.ranges[2 * f] = (int)o, D.ranges[2 * f + 1] = -1;
  }
  (void)s_go;
  if (stage == kSolve1) gather_frame(D, f, wsum, &s_base);
}

// The gates behind a solve (:342-349, :361-369, :375-387).  which = 1, 2, 3: the solve it follows.
__global__ __launch_bounds__(256) void k_reloc_after_solve(RelocDev D, int r, int which) {
  const int f = blockIdx.x, tid = threadIdx.x;
  int *rec = D.rec + (size_t)f * kRecInts;
  const int want = which == 1 ? kSolve1 : which == 2 ? kSolve2 : kSolve3;
  if (rec[kRecStage] != want) return;
  __syncthreads();  // (every thread has read the stage before thread 0 rewrites it)
  const int p = f * D.MC + r;
  const size_t o = (size_t)f * D.cap;
  const int inl = D.ninl_solve[f];
  const int start = D.ranges[2 * f], count = D.ranges[2 * f + 1];
  // frame->outliers_[idx] of the problem's features (optimizer_ceres.cpp:199, :284-302); the others keep their value
  const bool cull = which == 3 || (which == 1 && inl >= 10);
  for (int d = tid; d < count; d += 256) {
    const int i = D.index[start + d];
    const uint8_t out = D.outlier[start + d];
    D.foutl[o + i] = out;
    if (cull && out) D.fhas[o + i] = 0, D.fobs[o + i] = 0, D.fid[o + i] = -1;  // :345-349, :377-381
  }
  int stage = kIdle, code = -1;
  if (which == 1) {
    if (inl < 10) code = kOutFewSolve;      // :342-343
    else if (inl >= 50) code = kOutSuccess;  // :352, :387
    else stage = kTop1;
  } else if (which == 2) {
    if (inl > 30 && inl < 50) {  // :361-369: found = every map point the frame holds now
      uint8_t *found = D.found + (size_t)f * D.MC * D.NK;
      for (int i = tid; i < D.MC * D.NK; i += 256) found[i] = 0;
      __syncthreads();
      const int n = min(D.fn[f], D.cap);
      for (int i = tid; i < n; i += 256)
        if (D.fhas[o + i]) found[D.fid[o + i]] = 1;
      stage = kTop2;
    } else {
      code = inl >= 50 ? kOutSuccess : kOutBelow50;
    }
  } else {
    code = inl >= 50 ? kOutSuccess : kOutBelow50;
  }
  if (tid == 0) {
    rec[kRecInliers] = inl;
    rec[kRecStage] = stage;
    if (code >= 0) D.out_code[p] = code;
    if (code == kOutSuccess) rec[kRecDone] = 1, rec[kRecWinner] = r;
  }
}

// The projection prologue of searchByProjection(Frame*, KeyFrame*, radius, distThreshold, found) (matcher.cpp:165-203)
// for the key-frame features of candidate r, with Tcw = exp(pose) of the solve before (the sibling of k_track_in_frame:
// the same transform and narrowing; here z <= 0 fails, the distance gate is the point's own range, there is no view
// cosine, and a point whose id is in `found` is skipped).  which = 1, 2: the top-up it prepares.
__global__ __launch_bounds__(256) void k_reloc_project(RelocDev D, int r, int which, float fx, float fy, float cx, float cy,
                                                       int xmin, int xmax, int ymin, int ymax, float log_sf1, int n_levels) {
  __shared__ double s_T[10];
  const int f = blockIdx.y, tid = threadIdx.x, q = blockIdx.x * 256 + tid;
  const int *rec = D.rec + (size_t)f * kRecInts;
  const int p = f * D.MC + r;
  const bool go = rec[kRecStage] == (which == 1 ? kTop1 : kTop2);
  if (blockIdx.x == 0 && tid == 0) D.nq[f] = go ? D.kf_n[p] : -1;
  if (!go) return;
  {  // the search starts from "no feature assigned in this call"
    const size_t o = (size_t)f * D.cap;
    for (int i = q; i < D.cap; i += (int)gridDim.x * 256) D.assigned[o + i] = -1;
  }
  if (tid == 0) {
    const Se3 T = se3_exp(D.pose + 6 * (size_t)f);
    // Ow = Tcw.inverse().translation() (:166): the conjugate rotation of -t
    const double qc[4] = {T.q[0], -T.q[1], -T.q[2], -T.q[3]}, nt[3] = {-T.t[0], -T.t[1], -T.t[2]};
    double ow[3];
    quat_rotate(qc, nt, ow);
    for (int k = 0; k < 4; k++) s_T[k] = T.q[k];
    for (int k = 0; k < 3; k++) s_T[4 + k] = T.t[k], s_T[7 + k] = ow[k];
  }
  __syncthreads();
  if (q >= D.kf_n[p]) return;
  const size_t ko = (size_t)p * D.NK + q;
  uint8_t out = 0;
  float u = 0.f, v = 0.f;
  int level = 0;
  if ((D.kf_flags[ko] & 1u) && !D.found[(size_t)f * D.MC * D.NK + D.kf_id[ko]]) {  // :173-177
    const double *pw = D.kf_point + 3 * ko;
    const double qq[4] = {s_T[0], s_T[1], s_T[2], s_T[3]};
    double rp[3];
    quat_rotate(qq, pw, rp);
    const double x = rp[0] + s_T[4], y = rp[1] + s_T[5], zc = rp[2] + s_T[6];
    const float z = (float)zc;
    if (!(z <= 0.0f)) {  // :180-182
      u = (float)((double)fx * x / zc + (double)cx);  // Camera::camera2pixel, camera.cpp:72-75 (float members widened)
      v = (float)((double)fy * y / zc + (double)cy);
      if (!(u > xmax || u < xmin) && !(v > ymax || v < ymin)) {  // :188-191
        const double l0 = pw[0] - s_T[7], l1 = pw[1] - s_T[8], l2 = pw[2] - s_T[9];
        const float dist = (float)sqrt(l0 * l0 + l1 * l1 + l2 * l2);                // :193-194
        const float mind = 0.8f * D.kf_mind[ko], maxd = 1.2f * D.kf_maxd[ko];      // mappoint.cpp:391-401
        if (!(dist < mind || dist > maxd)) {                                       // :198
          out = 1;
          const float ratio = D.kf_maxd[ko] / dist;  // MapPoint::predictScale, mappoint.cpp:182-196
          const float lg = (float)log((double)ratio);
          const int s = (int)ceilf(lg / log_sf1);
          level = s < 0 ? 0 : (s >= n_levels ? n_levels - 1 : s);
        }
      }
    }
  }
  if (!out) u = v = 0.f, level = 0;
  D.qflags[ko] = out, D.qu[ko] = u, D.qv[ko] = v, D.qlevel[ko] = level;
}

// Behind a top-up search: its matches into the frame's slots (matcher.cpp:262-268 via `assigned`), then the gate
// `inliers_num_ + addition >= 50` (:357, :373): the frames that pass get the observation list of the next solve.
__global__ __launch_bounds__(256) void k_reloc_after_search(RelocDev D, int r, int which) {
  __shared__ int wsum[4];
  __shared__ int s_base;
  const int f = blockIdx.x, tid = threadIdx.x;
  int *rec = D.rec + (size_t)f * kRecInts;
  const size_t o = (size_t)f * D.cap;
  const bool go = rec[kRecStage] == (which == 1 ? kTop1 : kTop2);
  __syncthreads();
  if (!go) {
    if (tid == 0) D.ranges[2 * f] = (int)o, D.ranges[2 * f + 1] = -1;
    return;
  }
  const int p = f * D.MC + r;
  const size_t ko = (size_t)p * D.NK;
  const int n = min(D.fn[f], D.cap);
  for (int i = tid; i < n; i += 256) {
    const int a = D.assigned[o + i];
    if (a < 0) continue;
    const double *P3 = D.kf_point + 3 * (ko + a);
    D.fpoint[3 * (o + i)] = P3[0], D.fpoint[3 * (o + i) + 1] = P3[1], D.fpoint[3 * (o + i) + 2] = P3[2];
    D.fhas[o + i] = 1, D.fobs[o + i] = (D.kf_flags[ko + a] >> 1) & 1u, D.fid[o + i] = D.kf_id[ko + a];
  }
  const bool solve = rec[kRecInliers] + D.nm[f] >= 50;
  __syncthreads();
  if (tid == 0) {
    rec[kRecStage] = solve ? (which == 1 ? kSolve2 : kSolve3) : kIdle;
    if (!solve) D.out_code[p] = kOutBelow50, D.ranges[2 * f] = (int)o, D.ranges[2 * f + 1] = -1;
  }
  if (solve) gather_frame(D, f, wsum, &s_base);
}

// End of the walk: the status word and the frame's record of the result block (the layout of k_track_pack: pose,
// n_tracked, n_inliers, two match counts, status).
__global__ __launch_bounds__(256) void k_reloc_finish(RelocDev D, int *winner, uint8_t *resblk, const int *orb_err,
                                                      const int *guided_err) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= D.B) return;
  const int *rec = D.rec + (size_t)f * kRecInts;
  const bool ok = rec[kRecDone] != 0;
  winner[f] = ok ? rec[kRecWinner] : -1;
  double *pd = reinterpret_cast<double *>(resblk + (size_t)f * 72);
  for (int k = 0; k < 6; k++) pd[k] = D.pose[6 * f + k];
  int *pi = reinterpret_cast<int *>(resblk + (size_t)f * 72 + 48);
  const int inl = rec[kRecInliers];
  pi[0] = inl, pi[1] = inl, pi[2] = ok ? D.out_bow[f * D.MC + rec[kRecWinner]] : 0, pi[3] = 0;
  pi[4] = ok ? 0 : VO_TRACK_RELOC_FAILED, pi[5] = 0;
  if (f == 0) {
    int *fl = reinterpret_cast<int *>(resblk + (size_t)D.B * 72);
    fl[0] = orb_err ? *orb_err : 0;
    fl[1] = guided_err ? *guided_err : 0;
  }
}

// ---- the store routes: the candidates are key-frame numbers in device memory ------------------
enum { kErrTooMany = vo::kStoreErrTooMany, kErrBadId = vo::kStoreErrBadId };  // the sticky word of the store routes

struct StoreDev {
  vo::KfStoreView S;
  const int *n_cand_in, *cand_in;  // the caller's (or the database's) lists: [B], [B][cand_stride]
  int cand_stride;
  int *nc, *nc_true, *walked, *pair_kf;  // [B] walked / true counts, [B * MC] ids as given (-1 beyond), validated (-1: none)
  int *kf_n;                             // the Reloc arrays the dependent tail reads, written here
  uint8_t *kf_bad, *kf_flags;
  double *kf_point;
  int *kf_id;
  uint8_t *kf_pdesc;
  float *kf_mind, *kf_maxd, *kf_angle;
  int *l2g;    // [B][MC * NK] local id -> global id
  int *fid_g;  // [B][cap] the frame's ids at the end, global
  int *err;
};

// Candidate c of frame f: the chosen key-frame's record out of the store into the arrays of pair p = f * MC + c, in the
// layout reloc_set_candidates uploads -- the dependent tail runs unchanged.  A number outside the store makes the pair a
// bad key-frame without features and raises the sticky word; so does a frame with more candidates than MC (its first MC
// are walked).  The word is only ever OR-ed: its value does not depend on the order of the workgroups.
__global__ __launch_bounds__(256) void k_kfstore_gather(RelocDev D, StoreDev T) {
  const int p = blockIdx.x, f = p / D.MC, c = p % D.MC, tid = threadIdx.x;
  const int ntrue = T.n_cand_in[f], nc = min(max(ntrue, 0), min(D.MC, T.cand_stride));
  if (c == 0 && tid == 0) {
    T.nc[f] = nc, T.nc_true[f] = ntrue;
    if (ntrue > D.MC) atomicOr(T.err, kErrTooMany);
  }
  int raw = -1, k = -1;
  if (c < nc) {
    raw = T.cand_in[(size_t)f * T.cand_stride + c];
    if (raw >= 0 && raw < T.S.size) k = raw;
    else if (tid == 0) atomicOr(T.err, kErrBadId);
  }
  if (tid == 0) T.walked[p] = raw, T.pair_kf[p] = k;
  if (c >= nc) return;  // (the arrays of a pair beyond the frame's count are never read)
  if (k < 0) {
    if (tid == 0) T.kf_n[p] = 0, T.kf_bad[p] = 1;
    return;
  }
  const int *head = vo::kf_head(T.S, k);
  const int n = min(max(head[0], 0), D.NK);
  if (tid == 0) T.kf_n[p] = n, T.kf_bad[p] = head[1] != 0;
  const size_t ko = (size_t)p * D.NK;
  const uint8_t *flags = vo::kf_sec<uint8_t>(T.S, k, T.S.o_flags);
  const int *ids = vo::kf_sec<int>(T.S, k, T.S.o_ids);
  const float *mind = vo::kf_sec<float>(T.S, k, T.S.o_mind), *maxd = vo::kf_sec<float>(T.S, k, T.S.o_maxd);
  const float *angle = vo::kf_sec<float>(T.S, k, T.S.o_angle);
  const double *pts = vo::kf_sec<double>(T.S, k, T.S.o_points);
  const uint32_t *pd = vo::kf_sec<uint32_t>(T.S, k, T.S.o_pdesc);
  for (int i = tid; i < n; i += 256) {
    T.kf_flags[ko + i] = flags[i], T.kf_id[ko + i] = (flags[i] & 1) ? ids[i] : 0;  // (an unflagged feature's id is never read)
    T.kf_mind[ko + i] = mind[i], T.kf_maxd[ko + i] = maxd[i], T.kf_angle[ko + i] = angle[i];
  }
  for (int i = tid; i < 3 * n; i += 256) T.kf_point[3 * ko + i] = pts[i];
  uint32_t *opd = reinterpret_cast<uint32_t *>(T.kf_pdesc + ko * 32);
  for (int i = tid; i < 8 * n; i += 256) opd[i] = pd[i];
}

// MapPoint identity for the walk: `found` and fid are indexed by an id in [0, MC * NK), the store's ids are any
// non-negative int32.  One workgroup per frame: the flagged features of the frame's candidates as keys (global id << 32 |
// slot), slot = c * NK + i; sorted (distinct keys: one possible order), every feature's local id is the SMALLEST slot that
// carries its global id -- the head of its run, found by binary search.  Equal global ids get equal local ids, distinct
// ones distinct slots, all below MC * NK, and nothing depends on timing.  l2g keeps the way back.  Keys in LDS when the
// power of two above MC * NK fits (lds_slots), else in a slab of device memory owned by the frame.
__global__ __launch_bounds__(256) void k_reloc_local_ids(int MC, int NK, const int *nc, const int *kf_n, const uint8_t *kf_flags,
                                                         int *kf_id, int *l2g, unsigned long long *gkeys, int gstride, int lds_slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long li_keys[];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = min(max(nc[f], 0), MC) * NK, np2 = vo::pow2_ceil(M);
  if (M == 0) return;
  unsigned long long *keys = np2 <= lds_slots ? li_keys : gkeys + (size_t)f * gstride;
  const size_t fo = (size_t)f * MC * NK;
  for (int s = tid; s < np2; s += 256) {
    unsigned long long key = ~0ull;
    if (s < M) {
      const int c = s / NK, i = s - c * NK;
      if (i < kf_n[f * MC + c] && (kf_flags[fo + s] & 1)) key = ((unsigned long long)(unsigned)kf_id[fo + s] << 32) | (unsigned)s;
    }
    keys[s] = key;
  }
  vo::block_bitonic_sort(keys, np2);
  for (int j = tid; j < np2; j += 256) {
    const unsigned long long key = keys[j];
    if (key == ~0ull) continue;
    const unsigned long long first = key & 0xffffffff00000000ull;
    int lo = 0, hi = j;  // first position whose key is >= (id, slot 0): the head of the id's run
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < first) lo = mid + 1;
      else hi = mid;
    }
    const int local = (int)(keys[lo] & 0xffffffffu);
    kf_id[fo + (key & 0xffffffffu)] = local;
    if (lo == j) l2g[fo + local] = (int)(key >> 32);
  }
}

// behind k_reloc_finish: the frame's ids back as the store's, the sticky word into the result block (third flag)
__global__ __launch_bounds__(256) void k_reloc_store_finish(RelocDev D, StoreDev T, uint8_t *resblk) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)f * D.cap, fo = (size_t)f * D.MC * D.NK;
  for (int i = tid; i < D.cap; i += 256) {
    const int id = D.fid[o + i];
    T.fid_g[o + i] = id >= 0 && id < D.MC * D.NK ? T.l2g[fo + id] : -1;
  }
  if (f == 0 && tid == 0) reinterpret_cast<int *>(resblk + (size_t)D.B * 72)[2] = *T.err;
}

// Map::detectRelocalizationCandidates' query vectors: the frames' (word, weight) pairs out of the [B][cap] slots into the
// ragged layout vo_bow_vector_dev reads.  One workgroup scans the feature counts, one per frame copies.
__global__ __launch_bounds__(256) void k_reloc_word_start(int B, int cap, const int *fn, int *start) {
  __shared__ int s_sum[256];
  const int tid = threadIdx.x, per = (B + 255) / 256, b = min(tid * per, B), e = min(b + per, B);
  int s = 0;
  for (int i = b; i < e; i++) s += min(max(fn[i], 0), cap);
  s_sum[tid] = s;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; t++) base += s_sum[t];
  for (int i = b; i < e; i++) start[i] = base, base += min(max(fn[i], 0), cap);
  if (tid == 255) start[B] = base;
}
__global__ __launch_bounds__(256) void k_reloc_word_pack(int cap, const int *fn, const int *start, const int *w, const double *wt,
                                                         int *ow, double *owt) {
  const int f = blockIdx.x, n = min(max(fn[f], 0), cap), o = start[f];
  for (int i = threadIdx.x; i < n; i += 256) ow[o + i] = w[(size_t)f * cap + i], owt[o + i] = wt[(size_t)f * cap + i];
}

// ---- trackLocalMap behind a relocalisation (vo_tracker_track_local_map after vo_tracker_relocalize*): searchLocalMapPoints
// (visualOdometry.cpp:726-774) and the second solve with its count (:287-303) on the frame state the walk left.  A frame
// whose relocalisation failed takes no part: nq[f] = -1 leaves it out of every step and nothing of it is written.
struct LocalDev {
  int nq, stride;          // local points per frame, row stride
  const uint8_t *pf1;      // [B][stride] the local map's flags as set
  uint8_t *q1_flags;       // [B][stride] out: the flags Frame::isInFrame is run with (0: skipped)
  const int *ids1;         // [B][stride] map-point ids of the local points, or NULL: nothing is skipped
  const double *p1;
  int *fid;                // [B][cap] the frame's ids in the id space VO_TRACKER_RELOC_POINT_IDS reports
  const int *winner;
};

// `mp->visualIdxOfFrame_ == frame_curr_->id_` (:753) by id: the ids held by the frame's non-null, non-outlier slots are sorted
// in LDS (block_sort.h; the power of two above cap keys) and every local point looks its id up by binary search -- cap log cap
// + n_local log cap per frame instead of the cap x n_local of a scan per point.  Also clears `assigned` for the search.
__global__ __launch_bounds__(256) void k_reloc_local_prep(RelocDev D, LocalDev L) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long lp_keys[];
  const int f = blockIdx.x, tid = threadIdx.x;
  const bool active = L.winner[f] >= 0;
  if (tid == 0) D.nq[f] = active ? L.nq : -1;
  if (!active) return;
  const size_t o = (size_t)f * D.cap, lo = (size_t)f * L.stride;
  const int n = min(max(D.fn[f], 0), D.cap), np2 = vo::pow2_ceil(D.cap);
  for (int i = tid; i < D.cap; i += 256) D.assigned[o + i] = -1;
  if (L.ids1) {
    for (int s_ = tid; s_ < np2; s_ += 256) {
      unsigned long long key = ~0ull;
      if (s_ < n && D.fhas[o + s_] && !D.foutl[o + s_] && L.fid[o + s_] >= 0) key = (unsigned long long)(unsigned)L.fid[o + s_];
      lp_keys[s_] = key;
    }
    vo::block_bitonic_sort(lp_keys, np2);
  }
  for (int q = tid; q < L.nq; q += 256) {
    uint8_t pf = L.pf1[lo + q];
    if ((pf & 1u) && L.ids1) {
      const int id = L.ids1[lo + q];
      if (id >= 0) {
        const unsigned long long key = (unsigned long long)(unsigned)id;
        int a = 0, b = np2;  // first key >= id
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (lp_keys[mid] < key) a = mid + 1;
          else b = mid;
        }
        if (a < np2 && lp_keys[a] == key) pf = 0;
      }
    }
    L.q1_flags[lo + q] = pf;
  }
}

// the search's matches into the frame's slots (matcher.cpp:338-340), then the observation list of the solve over ALL
// non-null slots (:287)
__global__ __launch_bounds__(256) void k_reloc_local_gather(RelocDev D, LocalDev L) {
  __shared__ int wsum[4];
  __shared__ int s_base;
  const int f = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)f * D.cap, lo = (size_t)f * L.stride;
  if (D.nq[f] < 0) {
    if (tid == 0) D.ranges[2 * f] = (int)o, D.ranges[2 * f + 1] = -1;
    return;
  }
  const int n = min(max(D.fn[f], 0), D.cap);
  for (int i = tid; i < n; i += 256) {
    const int a = D.assigned[o + i];
    if (a < 0 || a >= L.nq) continue;
    const double *P3 = L.p1 + 3 * (lo + a);
    D.fpoint[3 * (o + i)] = P3[0], D.fpoint[3 * (o + i) + 1] = P3[1], D.fpoint[3 * (o + i) + 2] = P3[2];
    D.fhas[o + i] = 1, D.fobs[o + i] = (L.q1_flags[lo + a] >> 1) & 1u;
    L.fid[o + i] = L.ids1 ? L.ids1[lo + a] : -1;
  }
  __syncthreads();
  gather_frame(D, f, wsum, &s_base);
}

// outliers_ of the solve's features, inliers_num_ (:289-303: not outlier, and observed), the frame's record of the result
// block: pose, n_tracked, n_inliers = the solve's return value, n_matches_local; n_matches_last and the status stay
__global__ __launch_bounds__(256) void k_reloc_local_count(RelocDev D, uint8_t *resblk) {
  __shared__ int s4[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (D.nq[f] < 0) return;
  const size_t o = (size_t)f * D.cap;
  const int start = D.ranges[2 * f], count = D.ranges[2 * f + 1];
  int local = 0;
  for (int d = tid; d < count; d += 256) {
    const int i = D.index[start + d];
    const uint8_t out = D.outlier[start + d];
    D.foutl[o + i] = out;
    if (!out && D.fobs[o + i]) local++;
  }
  const int total = block_sum(local, s4);
  if (tid == 0) {
    double *pd = reinterpret_cast<double *>(resblk + (size_t)f * 72);
    for (int k = 0; k < 6; k++) pd[k] = D.pose[6 * f + k];
    int *pi = reinterpret_cast<int *>(resblk + (size_t)f * 72 + 48);
    pi[0] = total, pi[1] = D.ninl_solve[f], pi[3] = D.nm[f];
  }
}

struct CandHost {
  int n = 0;
  std::vector<uint8_t> valid, desc;
  std::vector<float> angle;
  std::vector<int32_t> node_id, start;
  std::vector<uint32_t> feat;
  vo_bow_view view{};
};

}  // namespace

struct vo::Reloc {
  int B = 0, cap = 0, MC = 0, NK = 0, n_levels = 0;
  float sf_host[16] = {0};
  const vo_vocab *vocab = nullptr;
  bool have = false;
  std::vector<CandHost> cands;  // [B * MC] (host: the common-node walk reads them)
  // The arrays, all sized from (B, cap, MC, NK) when the object is created: one block, laid out by layout().  `d` is the
  // kernels' view with this object's half filled in for good (reloc_dev adds the call's half); the arrays that no kernel reads
  // through RelocDev follow it.
  Arena mem;
  RelocDev d{};
  int *n_cand = nullptr, *winner = nullptr;  // [B] the counts vo_tracker_set_reloc_candidates uploaded; [B] k_reloc_finish's
  uint8_t *kf_pdesc = nullptr, *pnp_ws = nullptr;
  float *kf_angle = nullptr;
  size_t pnp_ws_bytes = 0;
  void layout(Arena &a);
  BowResidentBufs bow;
  OwnedPinnedBuf stage;
  // the store routes: their arrays are laid out by reloc_store_prepare on the first call of a store route (`s`: nc .. err and
  // the candidate arrays are set then, the rest per call), the database query's on the first call with a database
  bool store_ready = false, store_db = false, last_store = false;
  int ids_lds_slots = 0, ids_gstride = 0;
  BowWalkBufs *walk = nullptr;  // the tracker's (reloc_store_prepare)
  Arena store_mem, db_mem;
  StoreDev s{};
  unsigned long long *s_keys = nullptr;
  struct {
    int *fstart, *w, *bstart, *bw, *nc, *cand;
    double *wt, *bv;
  } q{};
  void layout_store(Arena &a);
  void layout_db(Arena &a);
};

void vo::Reloc::layout(Arena &a) {
  const size_t P = (size_t)B * MC, PK = P * NK, PC = P * cap, Bc = (size_t)B * cap;
  a.take(d.sf, 64);
  a.take(n_cand, B * 4 + 64);
  a.take(d.kf_n, P * 4 + 64);
  a.take(d.kf_bad, P + 64);
  a.take(d.kf_flags, PK);
  a.take(d.kf_point, PK * 24);
  a.take(d.kf_id, PK * 4);
  a.take(kf_pdesc, PK * 32);
  a.take(d.kf_mind, PK * 4);
  a.take(d.kf_maxd, PK * 4);
  a.take(kf_angle, PK * 4);
  a.take(d.bow_assigned, PC * 4);
  a.take(d.bow_n, P * 4 + 64);
  a.take(d.cnt, P * 4 + 64);
  a.take(d.off, P * 4 + 64);
  a.take(d.p3, PC * 12);
  a.take(d.p2, PC * 8);
  a.take(d.src, PC * 4);
  a.take(d.pnp_T, P * 96);
  a.take(d.pnp_mask, PC);
  a.take(d.pnp_n, P * 4 + 64);
  a.take(d.pnp_status, P * 4 + 64);
  a.take(pnp_ws, pnp_ws_bytes = vo_pnp_workspace_bytes((int)P, 100));
  a.take(d.dbg_mask, PC);
  a.take(d.rec, (size_t)B * kRecInts * 4);
  a.take(d.fid, Bc * 4);
  a.take(d.found, PK);
  a.take(d.out_bow, P * 4);
  a.take(d.out_pnp, P * 4);
  a.take(d.out_code, P * 4);
  a.take(d.nq, B * 4 + 64);
  a.take(d.qflags, PK);
  a.take(d.qu, PK * 4);
  a.take(d.qv, PK * 4);
  a.take(d.qlevel, PK * 4);
  a.take(d.ninl_solve, B * 4 + 64);
  a.take(winner, B * 4 + 64);
}

void vo::Reloc::layout_store(Arena &a) {
  const size_t P = (size_t)B * MC, PK = P * NK, Bc = (size_t)B * cap;
  a.take(s.nc, B * 4 + 64);
  a.take(s.nc_true, B * 4 + 64);
  a.take(s.walked, P * 4 + 64);
  a.take(s.pair_kf, P * 4 + 64);
  a.take(s.l2g, PK * 4);
  a.take(s.fid_g, Bc * 4);
  if (ids_gstride) a.take(s_keys, (size_t)B * ids_gstride * 8);  // (the id compaction's keys, when they do not fit in LDS)
}

void vo::Reloc::layout_db(Arena &a) {
  const size_t P = (size_t)B * MC, Bc = (size_t)B * cap;
  a.take(q.fstart, B * 4 + 64);
  a.take(q.w, Bc * 4);
  a.take(q.wt, Bc * 8);
  a.take(q.bstart, B * 4 + 64);
  a.take(q.bw, Bc * 4);
  a.take(q.bv, Bc * 8);
  a.take(q.nc, B * 4 + 64);
  a.take(q.cand, P * 4 + 64);
}

namespace {
RelocDev reloc_dev(vo::Reloc *r, const vo::RelocShared &S, const int *n_cand);
int reloc_tail(vo::Reloc *r, const vo::RelocShared &S, const RelocDev &D);
}  // namespace

namespace vo {

int reloc_create(Reloc **out, int B, int cap, int max_cand, int max_feat, const float *sf, int n_levels) {
  if (!out || B < 1 || cap < 1 || max_cand < 1 || max_feat < 1 || !sf || n_levels < 1 || n_levels > 16) return VO_ERR_INVALID;
  if ((long long)B * max_cand > VO_PNP_MAX_PROBLEMS || max_feat > 65534) {
    set_error("relocalisation route: %d frames x %d candidates exceed %d PnP problems, or %d features per candidate exceed 65534", B,
              max_cand, VO_PNP_MAX_PROBLEMS, max_feat);
    return VO_ERR_CAPACITY;
  }
  Reloc *r = new (std::nothrow) Reloc();
  if (!r) return VO_ERR_HIP;
  r->B = B, r->cap = cap, r->MC = max_cand, r->NK = max_feat, r->n_levels = n_levels;
  memcpy(r->sf_host, sf, (size_t)n_levels * 4);
  r->d.B = B, r->d.cap = cap, r->d.MC = max_cand, r->d.NK = max_feat;
  auto fill = [&]() -> int {
    VO_CHECK(r->mem.build([&](Arena &a) { r->layout(a); }, "relocalisation route"));
    float sf16[16] = {0};
    memcpy(sf16, sf, (size_t)n_levels * 4);
    VO_HIP_CHECK(hipMemcpy(r->d.sf, sf16, 64, hipMemcpyHostToDevice));
    return VO_OK;
  };
  const int rc = fill();
  if (rc != VO_OK) {
    reloc_destroy(r);
    return rc;
  }
  *out = r;
  return VO_OK;
}

void reloc_destroy(Reloc *r) { delete r; }

int reloc_set_candidates(Reloc *r, const vo_vocab *vocab, int max_cand, const int32_t *n_cand, const vo_reloc_candidate *cands,
                         hipStream_t st) {
  if (!r || !vocab || max_cand < 0 || !n_cand || (max_cand > 0 && !cands)) return VO_ERR_INVALID;
  const int B = r->B, MC = r->MC, NK = r->NK;
  // everything is validated BEFORE anything is enqueued or any state changes
  if (max_cand > MC) {
    set_error("vo_tracker_set_reloc_candidates: %d candidates per frame, the tracker holds %d (max_reloc_candidates)", max_cand, MC);
    return VO_ERR_CAPACITY;
  }
  for (int f = 0; f < B; f++) {
    if (n_cand[f] < 0 || n_cand[f] > max_cand) return VO_ERR_INVALID;
    for (int c = 0; c < n_cand[f]; c++) {
      const vo_reloc_candidate &K = cands[(size_t)f * max_cand + c];
      if (K.n < 0) return VO_ERR_INVALID;
      if (K.n > NK) {
        set_error("vo_tracker_set_reloc_candidates: frame %d candidate %d has %d features, the tracker holds %d (max_reloc_features)", f,
                  c, K.n, NK);
        return VO_ERR_CAPACITY;
      }
      if (K.n == 0) continue;
      const vo_bow_view *v = K.nodes;
      if (!K.angle || !K.desc || !v || !K.flags || !K.points || !K.ids || !K.point_desc || !K.min_distance || !K.max_distance ||
          v->n_nodes < 0 || (v->n_nodes > 0 && (!v->node_id || !v->start || !v->feat || v->start[0] != 0))) {
        set_error("vo_tracker_set_reloc_candidates: frame %d candidate %d lacks an array", f, c);
        return VO_ERR_INVALID;
      }
      for (int j = 0; j < v->n_nodes; j++)
        if (v->start[j + 1] < v->start[j]) return VO_ERR_INVALID;
      for (int i = 0, nf = v->n_nodes > 0 ? v->start[v->n_nodes] : 0; i < nf; i++)
        if ((int)v->feat[i] < 0 || (int)v->feat[i] >= K.n) return VO_ERR_INVALID;
      for (int i = 0; i < K.n; i++)
        if ((K.flags[i] & 1) && (K.ids[i] < 0 || K.ids[i] >= MC * NK)) {
          set_error("vo_tracker_set_reloc_candidates: frame %d candidate %d feature %d: id %d outside [0, %d)", f, c, i, K.ids[i],
                    MC * NK);
          return VO_ERR_INVALID;
        }
    }
  }
  const size_t P = (size_t)B * MC, PK = P * NK;
  // one staging block: n_cand | kf_n | bad | flags | id | mind | maxd | angle | point | pdesc
  const size_t o_nc = 0, o_n = o_nc + (size_t)B * 4, o_bad = o_n + P * 4, o_fl = (o_bad + P + 15) & ~(size_t)15,
               o_id = (o_fl + PK + 15) & ~(size_t)15, o_mind = o_id + PK * 4, o_maxd = o_mind + PK * 4, o_ang = o_maxd + PK * 4,
               o_pt = (o_ang + PK * 4 + 15) & ~(size_t)15, o_pd = o_pt + PK * 24, total = o_pd + PK * 32;
  VO_HIP_CHECK(hipStreamSynchronize(st));  // (a route still in flight reads the arrays replaced below)
  VO_CHECK(r->stage.reserve(total));
  uint8_t *h = r->stage.data();
  memset(h, 0, total);
  memcpy(h + o_nc, n_cand, (size_t)B * 4);
  std::vector<CandHost> host(P);
  for (int f = 0; f < B; f++)
    for (int c = 0; c < n_cand[f]; c++) {
      const vo_reloc_candidate &K = cands[(size_t)f * max_cand + c];
      const size_t p = (size_t)f * MC + c, ko = p * NK;
      reinterpret_cast<int *>(h + o_n)[p] = K.n;
      h[o_bad + p] = K.bad ? 1 : 0;
      if (K.n == 0) continue;
      const size_t n = (size_t)K.n;
      memcpy(h + o_fl + ko, K.flags, n);
      memcpy(h + o_id + ko * 4, K.ids, n * 4);
      memcpy(h + o_mind + ko * 4, K.min_distance, n * 4);
      memcpy(h + o_maxd + ko * 4, K.max_distance, n * 4);
      memcpy(h + o_ang + ko * 4, K.angle, n * 4);
      memcpy(h + o_pt + ko * 24, K.points, n * 24);
      memcpy(h + o_pd + ko * 32, K.point_desc, n * 32);
      if (K.bad) continue;  // (a bad candidate is never searched: its host copy stays empty)
      CandHost &H = host[p];
      H.n = K.n;
      H.valid.resize(n);
      for (size_t i = 0; i < n; i++) H.valid[i] = K.flags[i] & 1;
      H.desc.assign(K.desc, K.desc + n * 32), H.angle.assign(K.angle, K.angle + n);
      const vo_bow_view *v = K.nodes;
      if (v->n_nodes > 0) {
        H.node_id.assign(reinterpret_cast<const int32_t *>(v->node_id), reinterpret_cast<const int32_t *>(v->node_id) + v->n_nodes);
        H.start.assign(v->start, v->start + v->n_nodes + 1);
        H.feat.assign(v->feat, v->feat + v->start[v->n_nodes]);
      } else {
        H.start.assign(1, 0);
      }
      H.view.n_nodes = v->n_nodes, H.view.node_id = reinterpret_cast<const uint32_t *>(H.node_id.data());
      H.view.start = H.start.data(), H.view.feat = H.feat.data();
    }
  auto up = [&](void *d, size_t off, size_t bytes) -> int {
    VO_HIP_CHECK(hipMemcpyAsync(d, h + off, bytes, hipMemcpyHostToDevice, st));
    return VO_OK;
  };
  VO_CHECK(up(r->n_cand, o_nc, (size_t)B * 4));
  VO_CHECK(up(r->d.kf_n, o_n, P * 4));
  VO_CHECK(up(r->d.kf_bad, o_bad, P));
  VO_CHECK(up(r->d.kf_flags, o_fl, PK));
  VO_CHECK(up(r->d.kf_id, o_id, PK * 4));
  VO_CHECK(up(r->d.kf_mind, o_mind, PK * 4));
  VO_CHECK(up(r->d.kf_maxd, o_maxd, PK * 4));
  VO_CHECK(up(r->kf_angle, o_ang, PK * 4));
  VO_CHECK(up(r->d.kf_point, o_pt, PK * 24));
  VO_CHECK(up(r->kf_pdesc, o_pd, PK * 32));
  VO_HIP_CHECK(hipStreamSynchronize(st));  // the caller's arrays and the staging block are free again
  r->vocab = vocab;
  r->cands.swap(host);  // (the views point into the vectors' heap blocks, which move along with their owners)
  r->have = true;
  return VO_OK;
}

int reloc_run(Reloc *r, const RelocShared &S) {
  if (!r || !r->have) {
    set_error("vo_tracker_relocalize: no candidates (vo_tracker_set_reloc_candidates)");
    return VO_ERR_INVALID;
  }
  const int B = r->B, MC = r->MC, P = B * MC;
  hipStream_t st = S.st;
  // ---- independent front: searchByBoW of every pair (the call's one synchronisation is inside, after computeBow)
  std::vector<RefKeyFrame> kfs((size_t)P);
  for (int p = 0; p < P; p++) {
    const CandHost &k = r->cands[p];
    kfs[p] = RefKeyFrame{k.n, k.valid.data(), k.desc.data(), k.angle.data(), &k.view};
  }
  VO_CHECK(bow_search_resident(r->vocab, S.frames, 0, B, kfs.data(), 0.75f, 1, 3, r->d.bow_assigned, r->cap, r->d.bow_n, st, MC,
                               &r->bow));
  r->last_store = false;
  const RelocDev D = reloc_dev(r, S, r->n_cand);
  return reloc_tail(r, S, D);
}

}  // namespace vo

namespace {

// the device view of a route: the Reloc object's arrays (set when it was created) and the call's -- the per-frame counts the
// walk obeys, the frame store, the tracker's arrays
RelocDev reloc_dev(vo::Reloc *r, const vo::RelocShared &S, const int *n_cand) {
  const vo::FrameStoreView fs = vo::frame_store_view(S.frames);
  RelocDev D = r->d;
  D.fn = fs.n, D.X = fs.x, D.Y = fs.y, D.UR = fs.uright, D.OCT = fs.octave;
  D.n_cand = n_cand;
  D.pose = S.pose, D.fpoint = S.fpoint, D.fhas = S.fhas, D.foutl = S.foutl, D.fobs = S.fobs, D.pts = S.pts, D.obs = S.obs, D.isg = S.isg;
  D.ranges = S.ranges, D.index = S.index, D.outlier = S.outlier, D.assigned = S.assigned, D.nm = S.nm;
  return D;
}

// everything behind the BoW searches: the PnP of every pair, the dependent tail, the result block
int reloc_tail(vo::Reloc *r, const vo::RelocShared &S, const RelocDev &D) {
  const int B = r->B, MC = r->MC, NK = r->NK, P = B * MC;
  hipStream_t st = S.st;
  // ---- poseEstimateByPnP of every pair: ragged correspondence lists with device offsets, then the RANSAC
  hipLaunchKernelGGL(k_reloc_count, dim3(P), dim3(256), 0, st, D);
  hipLaunchKernelGGL(k_reloc_scan, dim3(1), dim3(256), 0, st, P, (const int *)D.cnt, D.off);
  hipLaunchKernelGGL(k_reloc_gather, dim3(P), dim3(256), 0, st, D);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(vo_pnp_ransac_dev(P, D.off, D.p3, D.p2, S.cam5, 100, 8.0f, 0.99, D.pnp_T, D.pnp_mask, D.pnp_n, D.pnp_status, nullptr,
                             r->pnp_ws, r->pnp_ws_bytes, st));
  hipLaunchKernelGGL(k_reloc_pnp_mask, dim3(P), dim3(256), 0, st, D);
  // ---- dependent tail
  vo_guided_queries q{};
  q.n_queries = NK, q.stride = MC * NK, q.n_per_frame = D.nq;
  vo_guided_params gp{};
  gp.mode = 2, gp.check_rot = 1, gp.n_levels = S.n_levels, gp.scale_factors = S.sf;
  const float log_sf1 = (float)log((double)S.sf[1]);
  auto solve = [&]() {
    return vo_pose_only_solve_ranges_dev(B, S.ranges, S.pts, S.obs, S.isg, S.cam5d, S.pose, S.outlier, D.ninl_solve, nullptr, st);
  };
  auto top_up = [&](int rd, int which, float radius, float dist_threshold) -> int {
    hipLaunchKernelGGL(k_reloc_project, dim3((NK + 255) / 256, B), dim3(256), 0, st, D, rd, which, S.cam5[0], S.cam5[1], S.cam5[2],
                       S.cam5[3], 0, S.width, 0, S.height, log_sf1, S.n_levels);
    VO_HIP_CHECK(hipGetLastError());
    const size_t ro = (size_t)rd * NK;  // query q of frame f = feature q of pair f * MC + rd: stride MC * NK from here
    q.flags = D.qflags + ro, q.u = D.qu + ro, q.v = D.qv + ro, q.level = D.qlevel + ro;
    q.angle = r->kf_angle + ro, q.desc = r->kf_pdesc + ro * 32;
    gp.radius = radius, gp.dist_threshold = dist_threshold;
    VO_CHECK(vo_match_guided_dev(S.frames, 0, B, &q, &gp, S.fhas, S.assigned, nullptr, S.nm, 0, st));
    hipLaunchKernelGGL(k_reloc_after_search, dim3(B), dim3(256), 0, st, D, rd, which);
    VO_HIP_CHECK(hipGetLastError());
    return VO_OK;
  };
  for (int rd = 0; rd < MC; rd++) {
    hipLaunchKernelGGL(k_reloc_apply, dim3(B), dim3(256), 0, st, D, rd);
    VO_HIP_CHECK(hipGetLastError());
    VO_CHECK(solve());  // :340
    hipLaunchKernelGGL(k_reloc_after_solve, dim3(B), dim3(256), 0, st, D, rd, 1);
    VO_CHECK(top_up(rd, 1, 10.f, 100.f));  // :355
    VO_CHECK(solve());                     // :359
    hipLaunchKernelGGL(k_reloc_after_solve, dim3(B), dim3(256), 0, st, D, rd, 2);
    VO_CHECK(top_up(rd, 2, 3.f, 60.f));  // :371
    VO_CHECK(solve());                   // :375
    hipLaunchKernelGGL(k_reloc_after_solve, dim3(B), dim3(256), 0, st, D, rd, 3);
    VO_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_reloc_finish, dim3((B + 255) / 256), dim3(256), 0, st, D, r->winner, S.resblk, S.orb_err, S.guided_err);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace

namespace vo {

const void *reloc_selector(const Reloc *r, int what, size_t *bytes) {
  if (!r) return nullptr;
  const size_t B = r->B, P = B * r->MC;
  switch (what) {
    case VO_TRACKER_RELOC_WINNER: *bytes = B * 4; return r->winner;
    case VO_TRACKER_RELOC_POINT_IDS: *bytes = B * r->cap * 4; return r->last_store ? r->s.fid_g : r->d.fid;
    case VO_TRACKER_RELOC_BOW_MATCHES: *bytes = P * 4; return r->d.out_bow;
    case VO_TRACKER_RELOC_PNP_INLIERS: *bytes = P * 4; return r->d.out_pnp;
    case VO_TRACKER_RELOC_OUTCOME: *bytes = P * 4; return r->d.out_code;
    case VO_TRACKER_RELOC_PNP_MASK: *bytes = P * r->cap; return r->d.dbg_mask;
    case VO_TRACKER_RELOC_CANDIDATES: *bytes = P * 4; return r->last_store ? r->s.walked : nullptr;
    case VO_TRACKER_RELOC_N_CANDIDATES: *bytes = B * 4; return r->last_store ? r->s.nc_true : nullptr;
    default: return nullptr;
  }
}

// ---- the store routes ------------------------------------------------------------------------------------------
int reloc_store_prepare(Reloc *r, BowWalkBufs *walk, int *err, bool with_db, hipStream_t st) {
  if (!r || !walk || !err) return VO_ERR_INVALID;
  r->walk = walk, r->s.err = err;
  if (!r->store_ready) {
    // the id compaction sorts the power of two above MC * NK keys per frame: in LDS up to 128 KiB, else in a slab
    const int np2 = pow2_ceil(r->MC * r->NK);
    if ((size_t)np2 * 8 <= 128 * 1024) {
      r->ids_lds_slots = np2, r->ids_gstride = 0;
      if ((size_t)np2 * 8 > 64 * 1024)
        VO_HIP_CHECK(hipFuncSetAttribute((const void *)k_reloc_local_ids, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    } else {
      r->ids_lds_slots = 0, r->ids_gstride = np2;
    }
    VO_CHECK(r->store_mem.build([&](Arena &a) { r->layout_store(a); }, "store route"));
    // the candidate arrays the gather writes in place of vo_tracker_set_reloc_candidates
    StoreDev &T = r->s;
    T.kf_n = r->d.kf_n, T.kf_bad = r->d.kf_bad, T.kf_flags = r->d.kf_flags, T.kf_point = r->d.kf_point, T.kf_id = r->d.kf_id;
    T.kf_pdesc = r->kf_pdesc, T.kf_mind = r->d.kf_mind, T.kf_maxd = r->d.kf_maxd, T.kf_angle = r->kf_angle;
    r->store_ready = true;
  }
  if (with_db && !r->store_db) {
    VO_CHECK(r->db_mem.build([&](Arena &a) { r->layout_db(a); }, "store route with a database"));
    r->store_db = true;
  }
  return VO_OK;
}

int reloc_run_store(Reloc *r, const RelocShared &S, const RelocStoreArgs &A) {
  if (!r || !r->store_ready || !A.store || !A.vocab || (A.db ? !r->store_db : (!A.dev_n_cand || !A.dev_cand || A.cand_stride < 0)))
    return VO_ERR_INVALID;
  const int B = r->B, MC = r->MC, NK = r->NK, P = B * MC;
  hipStream_t st = S.st;
  const FrameStoreView fs = frame_store_view(S.frames);
  hipEvent_t *ev = A.tev;
  auto mark = [&](int i) -> int {
    if (ev) VO_HIP_CHECK(hipEventRecord(ev[i], st));
    return VO_OK;
  };
  r->have = false;  // the candidate arrays are the store's from here: vo_tracker_relocalize needs its candidates set again
  r->last_store = true;
  // ---- Frame::computeBow and the frames' FeatureVectors
  VO_CHECK(bow_featvec_resident(A.vocab, S.frames, B, 3, *r->walk, st, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr));
  // ---- Map::detectRelocalizationCandidates: the frames' BoW vectors, the database query
  const int *n_cand = A.dev_n_cand, *cand = A.dev_cand;
  int stride = A.cand_stride;
  if (A.db) {
    hipLaunchKernelGGL(k_reloc_word_start, dim3(1), dim3(256), 0, st, B, r->cap, fs.n, r->q.fstart);
    hipLaunchKernelGGL(k_reloc_word_pack, dim3(B), dim3(256), 0, st, r->cap, fs.n, (const int *)r->q.fstart, (const int *)r->walk->w,
                       (const double *)r->walk->wt, r->q.w, r->q.wt);
    VO_HIP_CHECK(hipGetLastError());
    VO_CHECK(vo_bow_vector_dev(B, B * r->cap, r->q.fstart, r->q.w, r->q.wt, r->q.bstart, r->q.bw, r->q.bv, st));
    VO_CHECK(kfdb_query_reloc_on(A.db, st, B, r->q.bstart, r->q.bw, r->q.bv, A.dev_stale, MC, r->q.nc, r->q.cand));
    n_cand = r->q.nc, cand = r->q.cand, stride = MC;
  }
  // ---- the candidates out of the store, their ids made dense
  VO_CHECK(kfstore_order_before(A.store, st));
  const RelocDev D = reloc_dev(r, S, r->s.nc);
  StoreDev T = r->s;
  T.S = kfstore_view(A.store), T.n_cand_in = n_cand, T.cand_in = cand, T.cand_stride = stride;
  VO_CHECK(mark(2));
  hipLaunchKernelGGL(k_kfstore_gather, dim3(P), dim3(256), 0, st, D, T);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(mark(3));
  VO_CHECK(mark(4));
  hipLaunchKernelGGL(k_reloc_local_ids, dim3(B), dim3(256), (size_t)r->ids_lds_slots * 8, st, MC, NK, (const int *)T.nc,
                     (const int *)T.kf_n, (const uint8_t *)T.kf_flags, T.kf_id, T.l2g, r->s_keys,
                     r->ids_gstride, r->ids_lds_slots);
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(mark(5));
  // ---- searchByBoW of every pair: the common-node walk and the replay
  VO_CHECK(bow_walk_replay(S.frames, B, MC, T.S, T.pair_kf, 0.75f, 1, *r->walk, D.bow_assigned, D.bow_n, st,
                           ev ? ev[6] : nullptr, ev ? ev[7] : nullptr));
  VO_CHECK(reloc_tail(r, S, D));
  hipLaunchKernelGGL(k_reloc_store_finish, dim3(B), dim3(256), 0, st, D, T, S.resblk);
  VO_HIP_CHECK(hipGetLastError());
  return kfstore_order_after(A.store, st);
}

bool reloc_last_was_store(const Reloc *r) { return r && r->last_store; }

int reloc_frame_ids(Reloc *r, int **fid, const int **winner) {
  if (!r || !r->last_store || !fid || !winner) return VO_ERR_INVALID;
  *fid = r->s.fid_g, *winner = r->winner;
  return VO_OK;
}

// ---- trackLocalMap behind a relocalisation --------------------------------------------------------------------------
namespace {
LocalDev local_dev(Reloc *r, const RelocLocalArgs &L) {
  return LocalDev{L.nq, L.stride, L.pf1, L.q1_flags, L.ids1, L.p1, r->last_store ? r->s.fid_g : r->d.fid, r->winner};
}
}  // namespace

int reloc_local_prep(Reloc *r, const RelocShared &S, const RelocLocalArgs &L, const int **frame_on) {
  if (!r || !frame_on) return VO_ERR_INVALID;
  const size_t lds = (size_t)pow2_ceil(r->cap) * 8;
  if (lds > 128 * 1024) {
    set_error("vo_tracker_track_local_map: %d feature slots per frame, the id lookup sorts 16384", r->cap);
    return VO_ERR_CAPACITY;
  }
  if (lds > 64 * 1024)
    VO_HIP_CHECK(hipFuncSetAttribute((const void *)k_reloc_local_prep, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
  const RelocDev D = reloc_dev(r, S, r->n_cand);
  hipLaunchKernelGGL(k_reloc_local_prep, dim3(r->B), dim3(256), lds, S.st, D, local_dev(r, L));
  VO_HIP_CHECK(hipGetLastError());
  *frame_on = D.nq;
  return VO_OK;
}

int reloc_local_finish(Reloc *r, const RelocShared &S, const RelocLocalArgs &L) {
  if (!r) return VO_ERR_INVALID;
  const RelocDev D = reloc_dev(r, S, r->n_cand);
  hipLaunchKernelGGL(k_reloc_local_gather, dim3(r->B), dim3(256), 0, S.st, D, local_dev(r, L));
  VO_HIP_CHECK(hipGetLastError());
  VO_CHECK(vo_pose_only_solve_ranges_dev(r->B, S.ranges, S.pts, S.obs, S.isg, S.cam5d, S.pose, S.outlier, D.ninl_solve, nullptr, S.st));
  hipLaunchKernelGGL(k_reloc_local_count, dim3(r->B), dim3(256), 0, S.st, D, S.resblk);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

}  // namespace vo
