// pose_only.hip -- pose-only bundle adjustment on gfx950 (MI355X), FP64.
// Replaces myslam::Optimizer::solvePoseOnlySE3 (reference src/optimizer_ceres.cpp:157-314) together with the Ceres
// solve it delegates to (TrustRegionMinimizer + LevenbergMarquardtStrategy on one 6-dof pose; contract in DESIGN.md).
// One launch of k_pose_only per batch of frames: both LM rounds; the chi2 classification between them rides on round 1's
// first linearisation pass, the one behind round 1 runs on the passes' look-ahead.
#include "ba_math.h"
#include "vo_common.h"
#include "wave_ops.h"

#include <algorithm>
#include <type_traits>

namespace {

using namespace vo;
using namespace vo::ba;

// ============================================================================================
// Pose-only BA: Optimizer::solvePoseOnlySE3 (optimizer_ceres.cpp:157-314), one workgroup per frame
// ============================================================================================
struct PoseLm {
  double radius, decrease, x_cost, x_norm;
  int iterations, accepted, termination;
};

// A frame's observations (global memory, explicit address space: generic pointers in a struct turn every access
// into a flat load that waits for both counters).  Round 2 kept the first 768 of them in LDS in a compact form
// (one wavefront per SIMD cannot hide the latency of a load it waits for right away); with every load of a pass issued
// four trips ahead of its use the plain reads are as fast (0.284 against 0.286 ms per 1024 frames), and the 148 KB of
// LDS per CU the cache took go to the extraction kernels that run next to the solve (tracked step 4.39 -> 4.14 ms).
#define VO_GLOBAL __attribute__((address_space(1)))
constexpr int kPoseNd = 4;  // trips of 64 observations per register set of the one-wavefront pass (5 / 6: spills, round 3)
struct ObsView {
  const VO_GLOBAL double *pts, *obs, *isg;
  VO_GLOBAL uint8_t *outlier;  // the result, and the skip mask of a pass
  __device__ __forceinline__ void get(int i, double (&p)[3], double &ou, double &ov, double &our, double &is) const {
    p[0] = pts[3 * i], p[1] = pts[3 * i + 1], p[2] = pts[3 * i + 2];
    ou = obs[3 * i], ov = obs[3 * i + 1], our = obs[3 * i + 2];
    is = isg[i];
  }
};

// One observation's contribution to H (upper 21), g (6) and the cost; unscaled, loss-corrected.
//
// The pose Jacobian of edge_eval factors as J = A [I | X]: A = d r / d pc (rows u [a 0 c], v [0 b d], uR [a 0 e]) and
// X = -[pc]x, so with M = rho1 A^T A (3 x 3, M01 = 0) and m = rho1 A^T r
//     H += [ M    M X   ]      g += [ m     ]
//          [ .  X^T M X ]           [ X^T m ]
// and every column of X has two non-zeros: 15 + 14 + 12 multiply-adds and 14 adds for H (the dense row products of the
// 2-3 x 6 Jacobian: 60 + 15), the rotation half of J is never formed.
__device__ __forceinline__ void pose_obs_term(const PoseCache &P, const double (&pw)[3], double ou, double ov, double our,
                                              double is, const Cam &K, double hm, double hs, double (&acc)[28]) {
  // R p + t as three multiply-add chains that start from t (trans_point adds t last: a multiply and an add more per row)
  const double x = __builtin_fma(P.R[0], pw[0], __builtin_fma(P.R[1], pw[1], __builtin_fma(P.R[2], pw[2], P.t[0])));
  const double y = __builtin_fma(P.R[3], pw[0], __builtin_fma(P.R[4], pw[1], __builtin_fma(P.R[5], pw[2], P.t[1])));
  const double z = __builtin_fma(P.R[6], pw[0], __builtin_fma(P.R[7], pw[1], __builtin_fma(P.R[8], pw[2], P.t[2])));
  const double invz = inv_fast(z), invz2 = invz * invz;
  const bool stereo = !(our < 0);
  const double uhat = K.fx * x * invz + K.cx;
  const double r0 = (ou - uhat) * is;
  const double r1 = (ov - (K.fy * y * invz + K.cy)) * is;
  const double r2 = stereo ? (our - (uhat - K.bf * invz)) * is : 0.0;
  const double a = -invz * K.fx, b = -invz * K.fy, c = x * invz2 * K.fx, d = y * invz2 * K.fy;  // Jp[0], [7], [2], [8]
  const double a2 = stereo ? a : 0.0, e = stereo ? c - K.bf * invz2 : 0.0;                        // Jp[12], [14]
  const double s = r0 * r0 + r1 * r1 + r2 * r2;
  double rho0, rho1;
  huber(stereo ? hs : hm, s, rho0, rho1);
  acc[27] += 0.5 * rho0;
  const double wa = rho1 * a, wa2 = rho1 * a2, wb = rho1 * b, wc = rho1 * c, wd = rho1 * d, we = rho1 * e;
  const double M00 = __builtin_fma(wa, a, wa2 * a2), M02 = __builtin_fma(wa, c, wa2 * e), M11 = wb * b, M12 = wb * d;
  const double M22 = __builtin_fma(wc, c, __builtin_fma(wd, d, we * e));
  const double m0 = __builtin_fma(wa, r0, wa2 * r2), m1 = wb * r1, m2 = __builtin_fma(wc, r0, __builtin_fma(wd, r1, we * r2));
  // M X, X = [[0 z -y] [-z 0 x] [y -x 0]]
  const double X00 = y * M02, X10 = __builtin_fma(y, M12, -(z * M11)), X20 = __builtin_fma(y, M22, -(z * M12));
  const double X01 = __builtin_fma(z, M00, -(x * M02)), X11 = -(x * M12), X21 = __builtin_fma(z, M02, -(x * M22));
  const double X02 = -(y * M00), X12 = x * M11, X22 = __builtin_fma(x, M12, -(y * M02));
  // packed upper triangle, row by row: (0,b) 0..5, (1,b) 6..10, (2,b) 11..14, (3,b) 15..17, (4,b) 18..19, (5,5) 20
  acc[0] += M00, acc[2] += M02, acc[6] += M11, acc[7] += M12, acc[11] += M22;
  acc[3] += X00, acc[4] += X01, acc[5] += X02;
  acc[8] += X10, acc[9] += X11, acc[10] += X12;
  acc[12] += X20, acc[13] += X21, acc[14] += X22;
  // X^T (M X): column a of X against column b of M X
  acc[15] = __builtin_fma(y, X20, __builtin_fma(-z, X10, acc[15]));
  acc[16] = __builtin_fma(y, X21, __builtin_fma(-z, X11, acc[16]));
  acc[17] = __builtin_fma(y, X22, __builtin_fma(-z, X12, acc[17]));
  acc[18] = __builtin_fma(z, X01, __builtin_fma(-x, X21, acc[18]));
  acc[19] = __builtin_fma(z, X02, __builtin_fma(-x, X22, acc[19]));
  acc[20] = __builtin_fma(x, X12, __builtin_fma(-y, X02, acc[20]));
  acc[21] += m0, acc[22] += m1, acc[23] += m2;
  acc[24] = __builtin_fma(y, m2, __builtin_fma(-z, m1, acc[24]));
  acc[25] = __builtin_fma(z, m0, __builtin_fma(-x, m2, acc[25]));
  acc[26] = __builtin_fma(x, m1, __builtin_fma(-y, m0, acc[26]));
}

// float chi2 test of optimizer_ceres.cpp:262-303 (Q-B2: deliberately float)
__device__ __forceinline__ bool pose_chi2_outlier(const double pc[3], double ou, double ov, double our, float fx,
                                                  float fy, float cx, float cy, float bf, double isg) {
  const double x = pc[0], y = pc[1], z = pc[2];
  const float invz = (float)(1.0f / z);
  const float u = (float)(fx * x * invz + cx);
  const float v = (float)(fy * y * invz + cy);
  const float eu = (float)(u - ou), ev = (float)(v - ov);
  const float e2 = eu * eu + ev * ev;
  const float is2 = (float)(isg * isg);
  if (our < 0) return !(e2 * is2 < 5.991f);
  const float ur = u - bf * invz;
  const float eur = (float)(ur - our);
  return !((e2 + eur * eur) * is2 < 7.815f);
}

// The classification of a round: Tcw = exp(pose) (Sophus quaternion form, :256-257) and the float intrinsics.  The
// pose is the same in every lane: it is kept in scalar registers (a pass that classifies while it linearises has no
// fourteen vector registers to spare).
struct PoseCls {
  Se3 T;
  float fx, fy, cx, cy, bf;
};
__device__ __forceinline__ PoseCls pose_cls(const double x[6], const Cam &K) {
  const Se3 T = se3_exp(x);
  PoseCls C;
#pragma unroll
  for (int a = 0; a < 4; a++) C.T.q[a] = readlane_f64(T.q[a], 0);
#pragma unroll
  for (int a = 0; a < 3; a++) C.T.t[a] = readlane_f64(T.t[a], 0);
  C.fx = (float)K.fx, C.fy = (float)K.fy, C.cx = (float)K.cx, C.cy = (float)K.cy, C.bf = (float)K.bf;
  return C;
}
__device__ __forceinline__ bool pose_is_outlier(const PoseCls &C, const double (&pw)[3], double ou, double ov, double our, double is) {
  double rp[3], pc[3];
  quat_rotate(C.T.q, pw, rp);
  pc[0] = rp[0] + C.T.t[0], pc[1] = rp[1] + C.T.t[1], pc[2] = rp[2] + C.T.t[2];
  return pose_chi2_outlier(pc, ou, ov, our, C.fx, C.fy, C.cx, C.cy, C.bf, is);
}

// What a linearisation pass does with the flag array:
//   kPassAll       round 0: every observation takes part; no flag byte is loaded (the caller's buffer is not even cleared)
//   kPassFlags     round 1: flagged observations are skipped
//   kPassClassify  round 1's first pass, at x0: classifies every observation it holds at round 0's result, stores the
//                  flag and uses it as the skip bit -- round 0's classification read the same observations that this pass
//                  reads right behind it, in a loop of its own that waited for every load it issued
enum PosePass { kPassAll, kPassFlags, kPassClassify };

// A batch of observations of the one-wavefront form: ND trips of 64, in registers.
struct PoseOb { double pw[3], ou, ov, our, is; unsigned skip; };
// The loads take the wave-uniform bases from scalar registers and a 32-bit byte offset per lane (an int index costs
// twelve 64-bit address operations per observation); unconditional, the raw flag byte (FLAGS) included: a bool would be
// compared, i.e. waited for, where it is loaded.
template <bool FLAGS>
__device__ __forceinline__ void pose_request(const ObsView &V, unsigned base, unsigned last, PoseOb (&o)[kPoseNd]) {
  const unsigned lane = threadIdx.x;
  const VO_GLOBAL char *bp = (const VO_GLOBAL char *)V.pts, *bo = (const VO_GLOBAL char *)V.obs, *bi = (const VO_GLOBAL char *)V.isg;
  const VO_GLOBAL uint8_t *bs = V.outlier;
#pragma unroll
  for (int k = 0; k < kPoseNd; k++) {
    const unsigned i = min(base + 64u * k + lane, last);  // past the end: a harmless re-read
    const unsigned o24 = __umul24(i, 24u), o8 = i * 8u;  // (v_mul_lo_u32 is a quarter-rate instruction)
    o[k].pw[0] = *(const VO_GLOBAL double *)(bp + o24), o[k].pw[1] = *(const VO_GLOBAL double *)(bp + o24 + 8);
    o[k].pw[2] = *(const VO_GLOBAL double *)(bp + o24 + 16);
    o[k].ou = *(const VO_GLOBAL double *)(bo + o24), o[k].ov = *(const VO_GLOBAL double *)(bo + o24 + 8);
    o[k].our = *(const VO_GLOBAL double *)(bo + o24 + 16);
    o[k].is = *(const VO_GLOBAL double *)(bi + o8);
    o[k].skip = FLAGS ? bs[i] : 0u;
  }
}

// One linearisation pass over the observations that take part (PosePass).  WAVE (one wavefront per frame, nothing else on
// its SIMD to run while a load is in flight): observations travel in batches of four trips, one batch ahead of their
// use, into two register sets that swap roles in a loop unrolled by two (no "next becomes current" copies: 14 moves
// per observation).  `first` holds batch 0 on entry -- requested by the previous pass behind its last trip, so that it
// travels during the reduction and the 6 x 6 solve (the observations of a round do not change; a pass that requests
// its own first batch waits for it once per LM iteration) -- and again on exit; its flag bytes are there only where the
// next pass wants them (a classifying pass re-reads the ones it has just stored: same lane, same address, program order).
// kPassClassify adds its inliers to cnt: the wavefront's total (WAVE) or the lane's own (256-thread form).
template <bool WAVE, PosePass PASS>
__device__ __forceinline__ void pose_accumulate(const PoseCache &P, int n, const ObsView &V, const Cam &K, double hm, double hs,
                                                double (&acc)[28], PoseOb (&first)[kPoseNd], const PoseCls *C, int &cnt) {
#pragma unroll
  for (int i = 0; i < 28; i++) acc[i] = 0;
  if (WAVE) {
    const unsigned lane = threadIdx.x, last = (unsigned)(n - 1);
    constexpr int ND = kPoseNd;
    auto eval = [&](unsigned base, const PoseOb (&o)[ND]) {
#pragma unroll
      for (int k = 0; k < ND; k++) {
        const unsigned i = base + 64u * k + lane;
        bool use = i <= last;
        if (PASS == kPassFlags) use = use && !o[k].skip;
        if (PASS == kPassClassify) {
          const bool out = pose_is_outlier(*C, o[k].pw, o[k].ou, o[k].ov, o[k].our, o[k].is);
          if (use) V.outlier[i] = out ? 1 : 0;
          use = use && !out;
          cnt += __popcll(__ballot(use));
        }
        if (use) pose_obs_term(P, o[k].pw, o[k].ou, o[k].ov, o[k].our, o[k].is, K, hm, hs, acc);
      }
    };
    PoseOb B[ND];
#pragma unroll 1
    for (unsigned base = 0; base <= last; base += 2 * ND * 64) {
      pose_request<PASS == kPassFlags>(V, base + ND * 64, last, B);
      eval(base, first);
      const unsigned nb = base + 2 * ND * 64;
      pose_request<PASS != kPassAll>(V, nb > last ? 0u : nb, last, first);  // behind the last trip: batch 0 for the next pass (0.2275 -> 0.2235 ms)
      eval(base + ND * 64, B);  // (a batch wholly past the end evaluates nothing: every lane fails the range test)
    }
    return;
  }
#pragma unroll 1
  for (int i = threadIdx.x; i < n; i += (int)blockDim.x) {
    if (PASS == kPassFlags && V.outlier[i]) continue;
    double pw[3], ou, ov, our, is;
    V.get(i, pw, ou, ov, our, is);
    if (PASS == kPassClassify) {
      const bool out = pose_is_outlier(*C, pw, ou, ov, our, is);
      V.outlier[i] = out ? 1 : 0;
      if (out) continue;
      cnt++;
    }
    pose_obs_term(P, pw, ou, ov, our, is, K, hm, hs, acc);
  }
}

// The classification behind round 1: every observation against C, flags stored, inliers counted (WAVE: the wavefront's
// total; otherwise the lane's own).  No load is waited for in the trip that issues it: the one-wavefront form finds
// batch 0 in `first` (the last pass requested it) and keeps one batch of four trips in flight like a pass does; the
// 256-thread form requests a lane's next observation before it tests the present one.
template <bool WAVE>
__device__ __forceinline__ int pose_classify_all(int n, const ObsView &V, const PoseCls &C, PoseOb (&first)[kPoseNd]) {
  int cnt = 0;
  if (WAVE) {
    const unsigned lane = threadIdx.x, last = (unsigned)(n - 1);
    constexpr int ND = kPoseNd;
    auto cls = [&](unsigned base, const PoseOb (&o)[ND]) {
#pragma unroll
      for (int k = 0; k < ND; k++) {
        const unsigned i = base + 64u * k + lane;
        const bool out = pose_is_outlier(C, o[k].pw, o[k].ou, o[k].ov, o[k].our, o[k].is);
        if (i <= last) V.outlier[i] = out ? 1 : 0;
        cnt += __popcll(__ballot(i <= last && !out));
      }
    };
    PoseOb B[ND];
#pragma unroll 1
    for (unsigned base = 0; base <= last; base += 2 * ND * 64) {
      pose_request<false>(V, base + ND * 64, last, B);
      cls(base, first);
      const unsigned nb = base + 2 * ND * 64;
      if (nb <= last) pose_request<false>(V, nb, last, first);
      cls(base + ND * 64, B);
    }
    return cnt;
  }
  const int stride = (int)blockDim.x;
  int i = threadIdx.x;
  double pw[3], ou, ov, our, is;
  if (i < n) V.get(i, pw, ou, ov, our, is);
#pragma unroll 1
  for (; i < n; i += stride) {
    double npw[3], nou, nov, nour, nis;
    V.get(min(i + stride, n - 1), npw, nou, nov, nour, nis);  // past the end: a harmless re-read
    const bool out = pose_is_outlier(C, pw, ou, ov, our, is);
    V.outlier[i] = out ? 1 : 0;
    cnt += out ? 0 : 1;
    pw[0] = npw[0], pw[1] = npw[1], pw[2] = npw[2], ou = nou, ov = nov, our = nour, is = nis;
  }
  return cnt;
}

// 6 x 6 SPD solve on the packed lower triangle (row by row: 00 10 11 20 21 22 ...), in place; b := A^-1 b.  Fully
// unrolled (every index a compile-time constant: the 21 + 6 + 6 values stay in registers); no divide and no square
// root: per column one Newton-refined v_rsq_f64 (an ulp or two from 1 / sqrt(d), like the per-observation arithmetic),
// the column and both substitutions multiply by it -- 6 reciprocal square roots instead of 6 IEEE square roots and 33 IEEE
// divides (about 1000 of the 3600 instructions an LM iteration spent outside the observation loop).
__device__ __forceinline__ constexpr int tri_l(int i, int j) { return i * (i + 1) / 2 + j; }            // j <= i
__device__ __forceinline__ constexpr int tri_u(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }  // a <= b
__device__ __forceinline__ bool chol6_packed(double (&L)[21], double (&b)[6]) {
  double ri[6];  // 1 / L[j][j]
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = L[tri_l(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) d -= L[tri_l(j, k)] * L[tri_l(j, k)];
    if (!(d > 0.0)) return false;
    ri[j] = rsqrt_fast(d);
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double t = L[tri_l(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) t -= L[tri_l(i, k)] * L[tri_l(j, k)];
      L[tri_l(i, j)] = t * ri[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double t = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) t -= L[tri_l(i, k)] * b[k];
    b[i] = t * ri[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double t = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) t -= L[tri_l(k, i)] * b[k];
    b[i] = t * ri[i];
  }
  return true;
}

__device__ __forceinline__ void wave_lds_sync() {  // LDS hand-off between lanes of one wavefront
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// 64 lanes x 28 partial sums -> 28 totals at dst (LDS), in a fixed order: a transpose through LDS instead of 28 x 6
// DPP / readlane steps (about 110 instructions for what those did in 1000).  Layout: value-major, scratch[k][lane] at a
// pitch of kPoseRedPitch doubles -- a lane's stores of one value land on consecutive doubles across the wavefront.
//   ONE_PASS (the one-wavefront kernel, round 5): all 28 values in one trip: lane 2 v + h sums rows h, h + 2, ... of value v
//   (32 loads in flight, a pairwise tree), the halves meet by one quad permute.  Pitch 66: the reads of a half-wave fall on
//   banks 4 v + 4 j + 2 h (mod 64), all distinct.  One store / hand-off / load / hand-off chain per linearisation instead of two.
//   Two passes of 14 values (the 256-thread form: four scratch areas must fit next to each other): lane 4 v + q sums rows
//   q, q + 4, ..., two quad permutes; pitch 68: banks 8 v + 2 q + 8 j, distinct inside each half-wave (the lane-major
//   [64][15] layout of round 3 read two-way conflicted: 49 % of the kernel's LDS cycles).
// The hand-offs wait for LDS only where it matters: a wavefront-scope fence also waits for vmcnt(0).
template <bool ONE_PASS>
struct PoseRed {
  static constexpr int kPitch = ONE_PASS ? 66 : 68;
  static constexpr int kScratch = (ONE_PASS ? 28 : 14) * kPitch;
};
__device__ __forceinline__ void wave_lds_handoff() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // LDS only: the next pass's first batch stays in flight
  __builtin_amdgcn_wave_barrier();
}
template <bool ONE_PASS>
__device__ __forceinline__ void wave_reduce28(const double (&v)[28], double *scratch, double *dst) {
  constexpr int P = PoseRed<ONE_PASS>::kPitch;
  const int lane = threadIdx.x & 63;
  if (ONE_PASS) {
    const int vi = lane >> 1, h = lane & 1;
#pragma unroll
    for (int k = 0; k < 28; k++) scratch[k * P + lane] = v[k];
    wave_lds_handoff();
    double t = 0;
    if (lane < 56) {
      double u[32];
#pragma unroll
      for (int j = 0; j < 32; j++) u[j] = scratch[vi * P + 2 * j + h];
#pragma unroll
      for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
        for (int j = 0; j < w; j++) u[j] += u[j + w];
      t = u[0];
    }
    t += dpp_f64<0xB1>(t);  // quad_perm [1,0,3,2]
    if (lane < 56 && h == 0) dst[vi] = t;
    wave_lds_handoff();
    return;
  }
  const int vi = lane >> 2, q = lane & 3;
#pragma unroll
  for (int c = 0; c < 2; c++) {
#pragma unroll
    for (int k = 0; k < 14; k++) scratch[k * P + lane] = v[14 * c + k];
    wave_lds_handoff();
    double t = 0;
    if (lane < 56) {
      // all sixteen loads in flight before the first add (a running sum over loads waits for LDS once per term),
      // summed pairwise in a fixed order
      double u[16];
#pragma unroll
      for (int j = 0; j < 16; j++) u[j] = scratch[vi * P + 4 * j + q];
#pragma unroll
      for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
        for (int j = 0; j < w; j++) u[j] += u[j + w];
      t = u[0];
    }
    t += dpp_f64<0xB1>(t);  // quad_perm [1,0,3,2]
    t += dpp_f64<0x4E>(t);  // quad_perm [2,3,0,1]
    if (lane < 56 && q == 0) dst[14 * c + vi] = t;
    wave_lds_handoff();
  }
}

// LDS doubles of a pose-only workgroup behind the observation cache: the reduction scratch, the linearisation at x
// and at the candidate
template <bool WAVE>
struct PoseLds {
  static constexpr int kScratch = PoseRed<WAVE>::kScratch;
  static constexpr int kRed = WAVE ? kScratch : 4 * kScratch + 4 * 28;  // per-wave scratch, then the wave totals
  double red[kRed];
  double acc[28];   // linearisation at x: 21 + 6 + 1 sums, uniform over the workgroup
  double cand[28];  // ... at the trial point
};

// -DVO_POSE_STAMPS (tools/pose_stamps.py): shader-clock cycles per phase of the LM loop, summed over the iterations and
// handed back in the summary's fields (initial_cost = solve, final_cost = plus, final_radius = pass, reserved = reduction,
// accepted = tests) -- a developer build, never the product.  What lies outside the LM loops travels in the fields that
// are left: termination of the first summary = kernel entry to round 0's solve, of the second = the classification
// behind round 1; bits 8.. of the second summary's iterations = end of round 0's loop to the first iteration of round 1
// (the classification at round 0's result and round 1's first linearisation, in one pass or in two), of the first's = the
// whole kernel.
#ifdef VO_POSE_STAMPS
#define POSE_NOW(var, dep) asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(var), "+v"(dep)::"memory")
#define POSE_STAMP(slot, dep)                                                                            \
  do {                                                                                                   \
    unsigned long long t_;                                                                               \
    asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_), "+v"(dep)::"memory");                 \
    if ((slot) >= 0) st_[(slot) < 0 ? 0 : (slot)] += t_ - tp_;                                           \
    tp_ = t_;                                                                                            \
  } while (0)
#else
#define POSE_STAMP(slot, dep) do { } while (0)
#endif

// Ceres-style LM on one 6-dof pose.  The linearisations -- 21 + 6 + 1 sums each -- live in LDS, not in registers: a
// trial step accumulates the candidate's sums while the solve's temporaries are dead and vice versa (round 2 kept
// two sets of 28 accumulators next to a 6 x 6 system in every lane: 256 VGPR + 251 AGPR).  Every thread carries the
// (uniform) trust-region scalars in registers.
//
// ROUND 0 (Huber): no pass looks at the flag array.  ROUND 1 (plain): the first pass, at x0, is the classification at
// round 0's result C as well (kPassClassify) and leaves the inlier count in inl; below 10 (:306-307) the linearisation is
// dropped, nothing else is done and false comes back: the frame keeps round 0's pose.  `first` is batch 0 of the
// observations on entry and on exit (one-wavefront form).
template <bool WAVE, int ROUND>
__device__ __forceinline__ bool pose_lm(double x[6], int n, const ObsView &V, const Cam &K, double hm, double hs, int max_it,
                                        PoseLds<WAVE> &S, PoseOb (&first)[kPoseNd], const PoseCls *C, int *s_cnt, int &inl,
                                        vo_lm_summary *sum, unsigned long long *t_loop_) {
  // exp(x) is kept across the iterations (an accepted candidate's exp is the product se3_plus forms anyway) and the
  // residuals are evaluated from it: rotation matrix from the unit quaternion, t = V * upsilon -- what
  // se3TransPoint(x) computes through sin / cos of |omega|, up to rounding; no trigonometry per evaluation.
  Se3 Tx = se3_exp<true>(x);
#ifdef VO_POSE_STAMPS
  unsigned long long st_[5] = {0, 0, 0, 0, 0}, tp_ = 0;
#endif
  bool in_loop_ = false;  // (stamps)
  int cnt = 0;
  constexpr PosePass kFirstPass = ROUND == 0 ? kPassAll : kPassClassify, kLoopPass = ROUND == 0 ? kPassAll : kPassFlags;
  auto linearize = [&](auto pass, const Se3 &T, double *dst) {  // sums of the linearisation at T -> dst (LDS)
    double v[28];
    pose_accumulate<WAVE, decltype(pass)::value>(pose_cache_se3(T), n, V, K, hm, hs, v, first, C, cnt);
    POSE_STAMP(in_loop_ ? 2 : -1, v[27]);
    if (WAVE) {
      wave_reduce28<true>(v, S.red, dst);
    } else {
      // every wavefront reduces its lanes through its own scratch (the same transpose as the one-wavefront kernel: a
      // tenth of the instructions of 28 DPP / readlane sums -- this path is the latency of ONE frame), then 28 threads add
      // the wave totals in wave order
      const int wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
      constexpr int kS = PoseLds<WAVE>::kScratch;
      double *tot = S.red + 4 * kS;
      __syncthreads();  // the previous pass's totals have been read
      wave_reduce28<false>(v, S.red + wave * kS, tot + wave * 28);
      __syncthreads();
      if (threadIdx.x < 28) {
        double t = 0;
        for (int w = 0; w < nw; w++) t += tot[w * 28 + threadIdx.x];
        dst[threadIdx.x] = t;
      }
      __syncthreads();
    }
  };
  // the linearisation at x and the one at the candidate swap roles when a step is accepted (no copy)
  double *cur = S.acc, *cnd = S.cand;
  linearize(std::integral_constant<PosePass, kFirstPass>(), Tx, cur);
  if (ROUND == 1) {
    if (WAVE) {
      inl = cnt;
    } else {
      for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
      if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
      __syncthreads();
      inl = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
    if (inl < 10) return false;
  }
  double scale[6];
#pragma unroll
  for (int a = 0; a < 6; a++) scale[a] = 1.0 / (1.0 + sqrt(cur[tri_u(a, a)]));
  // The trust-region scalars: radius and decrease with their reciprocals next to them (decrease is a power of two, so
  // radius * inv_decrease is the quotient exactly; 1 / radius is refreshed when an accepted step changes the radius) --
  // the damping of an iteration is six multiplications, not six IEEE divisions in front of the factorisation.
  double radius = 1e4, inv_radius = 1e-4, decrease = 2.0, inv_decrease = 0.5, x_cost = cur[27];
  const double initial_cost = x_cost;
  auto norm6 = [](const double (&v)[6]) {
    const double s2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3] + v[4] * v[4] + v[5] * v[5];
    return s2 > 1e-280 ? s2 * rsqrt_fast(s2) : 0.0;  // (|x| below 1e-140 counts as zero: the test adds 1e-8 to it)
  };
  double x_norm;
  {
    const double xv[6] = {x[0], x[1], x[2], x[3], x[4], x[5]};
    x_norm = norm6(xv);
  }
  int iterations = 0, accepted = 0, termination = 0, invalid = 0;
  bool last_ok = false;
  for (int it = 1;; it++) {
    if (it - 1 >= max_it) {
      termination = 0;
      break;
    }
    in_loop_ = true;
    POSE_STAMP(-1, x_cost);
#ifdef VO_POSE_STAMPS
    if (t_loop_ && it == 1) *t_loop_ = tp_;
#endif
    double h[27];  // one batch of LDS reads: the gradient test and the normal equations use the same values
#pragma unroll
    for (int i = 0; i < 27; i++) h[i] = cur[i];
    if (last_ok) {
      double gm = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) gm = fmax(gm, fabs(h[21 + a]));
      if (gm <= 1e-10) {
        termination = 3;
        break;
      }
    }
    if (radius < 1e-32) {
      termination = 4;
      break;
    }
    iterations = it;
    last_ok = false;
    // scaled normal equations  H'' = S H S, g'' = S g ; LM diagonal from clamp(diag H'')/radius
    double L[21], g[6], y[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b2 = 0; b2 <= a; b2++) L[tri_l(a, b2)] = h[tri_u(b2, a)] * scale[b2] * scale[a];
      g[a] = h[21 + a] * scale[a];
      y[a] = g[a];
    }
    double model = 0, delta[6];
    {
      // step^T H'' step from the undamped matrix, before the factorisation overwrites it
      double Hs[21];
#pragma unroll
      for (int i = 0; i < 21; i++) Hs[i] = L[i];
#pragma unroll
      for (int a = 0; a < 6; a++) L[tri_l(a, a)] += fmin(fmax(L[tri_l(a, a)], 1e-6), 1e32) * inv_radius;
      bool ok = chol6_packed(L, y);
      if (ok) {
        double gs = 0, sHs = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
          if (!isfinite(y[a])) ok = false;
#pragma unroll
        for (int a = 0; a < 6; a++) {
          gs -= g[a] * y[a];  // step = -y
          double row = 0;
#pragma unroll
          for (int b2 = 0; b2 < 6; b2++) row += Hs[a >= b2 ? tri_l(a, b2) : tri_l(b2, a)] * y[b2];
          sHs += y[a] * row;
          delta[a] = -y[a] * scale[a];
        }
        model = -(gs + 0.5 * sHs);  // -m.(r + m/2) with m = J''step
      }
      if (!ok || !(model > 0.0)) {
        if (++invalid >= 5) {
          termination = 4;
          break;
        }
        radius *= inv_decrease, inv_radius *= decrease;
        decrease *= 2.0, inv_decrease *= 0.5;
        continue;
      }
    }
    invalid = 0;
    POSE_STAMP(0, model);
    double xc[6];
    Se3 Tc;
    se3_plus_keep(Tx, delta, xc, Tc);
    POSE_STAMP(1, xc[0]);
    // The candidate is linearised completely in the same pass (its cost is one of the 28 sums): an
    // accepted step -- the common case -- then needs no second sweep over the observations.
    linearize(std::integral_constant<PosePass, kLoopPass>(), Tc, cnd);
    double cand = cnd[27];
    POSE_STAMP(3, cand);
    if (!isfinite(cand)) cand = 1.7976931348623157e308;
    double sn = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) sn += (x[a] - xc[a]) * (x[a] - xc[a]);
    {
      const double tol = 1e-8 * (x_norm + 1e-8);  // |step| <= tol, compared as squares (no square root)
      if (sn <= tol * tol) {
        termination = 2;
        break;
      }
    }
    const double change = x_cost - cand;
    if (fabs(change) <= 1e-6 * x_cost) {
      termination = 1;
      break;
    }
    const double rel = change * inv_fast(model);
    if (rel > 1e-3) {
#pragma unroll
      for (int a = 0; a < 6; a++) x[a] = xc[a];
      Tx = Tc;
      x_norm = norm6(xc);
      double *t = cur;
      cur = cnd, cnd = t;  // the candidate's linearisation becomes the current one
      x_cost = cand;
      const double t2 = 2.0 * rel - 1.0;
      radius = fmin(radius * inv_fast(fmax(1.0 / 3.0, 1.0 - t2 * t2 * t2)), 1e16);
      inv_radius = inv_fast(radius);
      decrease = 2.0, inv_decrease = 0.5;
      accepted++;
      last_ok = true;
    } else {
      radius *= inv_decrease, inv_radius *= decrease;
      decrease *= 2.0, inv_decrease *= 0.5;
    }
    POSE_STAMP(4, radius);
  }
  if (sum && threadIdx.x == 0) {
    sum->iterations = iterations;
    sum->accepted = accepted;
    sum->termination = termination;
    sum->reserved = 0;
    sum->initial_cost = initial_cost;
    sum->final_cost = x_cost;
    sum->final_radius = radius;
#ifdef VO_POSE_STAMPS
    sum->initial_cost = (double)st_[0], sum->final_cost = (double)st_[1], sum->final_radius = (double)st_[2];
    sum->reserved = (int)st_[3], sum->accepted = (int)st_[4];
#endif
  }
  return true;
}

// ranges != 0: problem p owns observations [offsets[2p], offsets[2p] + offsets[2p+1]) (frames at a fixed stride,
// vo_track_gather_dev); otherwise [offsets[p], offsets[p+1]).  WAVE: one wavefront per problem (batches); otherwise
// 128 or 256 threads per problem (a few problems: the observations are shared out).
template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void k_pose_only(const int *offsets, const double *pts, const double *obs,
                                                               const double *isg, const double *cam5, double *poses,
                                                               uint8_t *outlier, int *n_inliers, vo_lm_summary *sums,
                                                               int ranges) {
  __shared__ PoseLds<WAVE> S;
  __shared__ int s_cnt[4];
  const int p = blockIdx.x;
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;  // (workgroups of one wavefront leave three of the four slots unused)
  const int o0 = ranges ? offsets[2 * p] : offsets[p], n = ranges ? offsets[2 * p + 1] : offsets[p + 1] - o0;
  pts += 3 * (long long)o0, obs += 3 * (long long)o0, isg += o0, outlier += o0;
  Cam K{cam5[0], cam5[1], cam5[2], cam5[3], cam5[4]};
  double x0[6], x[6];
  for (int a = 0; a < 6; a++) x0[a] = x[a] = poses[6 * p + a];
  if (n <= 0) {  // :204-205
    if (threadIdx.x == 0) n_inliers[p] = 0;
    return;
  }
  const ObsView V{(const VO_GLOBAL double *)pts, (const VO_GLOBAL double *)obs, (const VO_GLOBAL double *)isg, (VO_GLOBAL uint8_t *)outlier};
  // The flag array is written, never cleared: round 0 does not look at it, and round 1's first pass stores every byte
  // before anything reads one.
#ifdef VO_POSE_STAMPS
  unsigned long long t_in_ = 0, t_a_ = 0, t_b_ = 0, t_c_ = 0, t_end_ = 0, t_l1_ = 0;
  unsigned long long *const tl1_ = &t_l1_;  // (a frame that leaves after round 0 hands back no outer stamps: its second summary is zeroed)
  POSE_NOW(t_in_, x[0]);
#else
  unsigned long long *const tl1_ = nullptr;
#endif
  PoseOb first[kPoseNd];  // batch 0 of the frame's observations: every pass finds it in flight or arrived (one-wavefront form)
  if (WAVE) pose_request<false>(V, 0, (unsigned)(n - 1), first);
  int inl = 0;
#ifdef VO_POSE_STAMPS
  POSE_NOW(t_a_, x[0]);
#endif
  pose_lm<WAVE, 0>(x, n, V, K, (double)sqrtf(5.991f), (double)sqrtf(7.815f), 10, S, first, nullptr, s_cnt, inl,
                   sums ? &sums[2 * p] : nullptr, nullptr);
#ifdef VO_POSE_STAMPS
  POSE_NOW(t_b_, x[0]);
#endif
  // round 1 starts from x0 again (:215); its first pass classifies at round 0's result
  const PoseCls C0 = pose_cls(x, K);
  if (pose_lm<WAVE, 1>(x0, n, V, K, 0.0, 0.0, 10, S, first, &C0, s_cnt, inl, sums ? &sums[2 * p + 1] : nullptr, tl1_)) {
#pragma unroll
    for (int a = 0; a < 6; a++) x[a] = x0[a];
#ifdef VO_POSE_STAMPS
    POSE_NOW(t_c_, x[0]);
#endif
    const PoseCls C1 = pose_cls(x, K);
    int local = pose_classify_all<WAVE>(n, V, C1, first);
    if (WAVE) {
      inl = local;
    } else {
      for (int o = 32; o >= 1; o >>= 1) local += __shfl_xor(local, o);
      __syncthreads();  // round 1's count has been read
      if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = local;
      __syncthreads();
      inl = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
#ifdef VO_POSE_STAMPS
    double dep_ = (double)inl;
    POSE_NOW(t_end_, dep_);
    if (sums && threadIdx.x == 0) {
      sums[2 * p].termination = (int)(t_a_ - t_in_), sums[2 * p + 1].termination = (int)(t_end_ - t_c_);
      sums[2 * p].iterations |= (int)(t_end_ - t_in_) << 8, sums[2 * p + 1].iterations |= (int)(t_l1_ - t_b_) << 8;
    }
#endif
  } else if (sums && threadIdx.x == 0) {
    memset(&sums[2 * p + 1], 0, sizeof(vo_lm_summary));  // fewer than 10 inliers after round 0: round 1 did not run
  }
  if (threadIdx.x == 0) {
    n_inliers[p] = inl;
    for (int a = 0; a < 6; a++) poses[6 * p + a] = x[a];
  }
}

}  // namespace

extern "C" {

// The kernel is a chain of ~20 dependent LM iterations whose fixed part (6 x 6 solve, exp / log, reductions) every
// wavefront of a workgroup repeats, and it needs all 256 registers (one wavefront per SIMD).  A single frame is
// fastest with four wavefronts sharing its observations; a batch is fastest with ONE wavefront per frame, so that a
// CU works on four frames at once instead of four times on one (1024 frames x 1000 observations: 1.45 -> see DESIGN).
static inline int pose_block_width(int n_problems) {
  const int forced = vo::opt_pose_block();  // vo_set_option(VO_OPT_POSE_BLOCK, ...)
  if (forced == 64 || forced == 128 || forced == 256) return forced;
  return n_problems >= 512 ? 64 : 256;
}

int vo_pose_only_solve_dev(int n_problems, const int32_t *dev_offsets, int max_obs, const double *dev_points,
                           const double *dev_obs, const double *dev_inv_sigma, const double *dev_cam5,
                           double *dev_poses, uint8_t *dev_outlier, int32_t *dev_n_inliers,
                           vo_lm_summary *dev_summaries, void *hip_stream) {
  (void)max_obs;
  if (n_problems < 0 || (n_problems > 0 && (!dev_offsets || !dev_poses || !dev_outlier || !dev_n_inliers || !dev_cam5)))
    return VO_ERR_INVALID;
  if (n_problems == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  const int bw = pose_block_width(n_problems);
  hipLaunchKernelGGL(bw == 64 ? k_pose_only<true> : k_pose_only<false>, dim3(n_problems), dim3(bw), 0, (hipStream_t)hip_stream,
                     dev_offsets, dev_points, dev_obs, dev_inv_sigma, dev_cam5, dev_poses, dev_outlier, dev_n_inliers, dev_summaries, 0);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_pose_only_solve_ranges_dev(int n_problems, const int32_t *dev_ranges, const double *dev_points, const double *dev_obs,
                                  const double *dev_inv_sigma, const double *dev_cam5, double *dev_poses,
                                  uint8_t *dev_outlier, int32_t *dev_n_inliers, vo_lm_summary *dev_summaries,
                                  void *hip_stream) {
  if (n_problems < 0 || (n_problems > 0 && (!dev_ranges || !dev_poses || !dev_outlier || !dev_n_inliers || !dev_cam5)))
    return VO_ERR_INVALID;
  if (n_problems == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  const int bw = pose_block_width(n_problems);
  hipLaunchKernelGGL(bw == 64 ? k_pose_only<true> : k_pose_only<false>, dim3(n_problems), dim3(bw), 0, (hipStream_t)hip_stream,
                     dev_ranges, dev_points, dev_obs, dev_inv_sigma, dev_cam5, dev_poses, dev_outlier, dev_n_inliers, dev_summaries, 1);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_pose_only_solve(int n_problems, const int32_t *offsets, const double *points, const double *obs,
                       const double *inv_sigma, const double cam[5], double *poses, uint8_t *outlier,
                       int32_t *n_inliers, vo_lm_summary *summaries) {
  if (n_problems < 0 || (n_problems > 0 && (!offsets || !poses || !n_inliers || !cam))) return VO_ERR_INVALID;
  if (n_problems == 0) return VO_OK;
  VO_CHECK(vo::ensure_device());
  const int total = offsets[n_problems];
  if (total > 0 && (!points || !obs || !inv_sigma || !outlier)) return VO_ERR_INVALID;
  // One staging block each way (a tracking thread calls this once or twice per frame: eleven small
  // copies cost more than the kernel's first LM iterations).  Per host thread, grow-only.
  auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
  const size_t o_pts = 0, o_obs = o_pts + (size_t)total * 24, o_is = o_obs + (size_t)total * 24,
               o_cam = o_is + (size_t)total * 8, o_pose = o_cam + 40, o_off = o_pose + (size_t)n_problems * 48,
               in_bytes = up8(o_off + (size_t)(n_problems + 1) * 4);
  const size_t r_pose = 0, r_sum = r_pose + (size_t)n_problems * 48,
               r_inl = r_sum + (size_t)n_problems * 2 * sizeof(vo_lm_summary), r_out = up8(r_inl + (size_t)n_problems * 4),
               out_bytes = up8(r_out + (size_t)std::max(total, 1));
  hipStream_t st = vo::thread_stream();  // the calling thread's own stream: never queues behind another thread's solve
  thread_local vo::PinnedBuf pinned;
  thread_local vo::ScratchBuf d_in, d_out;
  VO_CHECK(pinned.reserve(std::max(in_bytes, out_bytes)));
  uint8_t *stage = pinned.data();
  if (total > 0) {
    memcpy(&stage[o_pts], points, (size_t)total * 24);
    memcpy(&stage[o_obs], obs, (size_t)total * 24);
    memcpy(&stage[o_is], inv_sigma, (size_t)total * 8);
  }
  memcpy(&stage[o_cam], cam, 40);
  memcpy(&stage[o_pose], poses, (size_t)n_problems * 48);
  memcpy(&stage[o_off], offsets, (size_t)(n_problems + 1) * 4);
  VO_CHECK(d_in.reserve(in_bytes));
  VO_CHECK(d_out.reserve(out_bytes));
  VO_HIP_CHECK(hipMemcpyAsync(d_in.p, stage, in_bytes, hipMemcpyHostToDevice, st));
  uint8_t *di = d_in.as<uint8_t>(), *dout = d_out.as<uint8_t>();
  // the kernel updates poses in place: give it the output block's copy
  VO_HIP_CHECK(hipMemcpyAsync(dout + r_pose, di + o_pose, (size_t)n_problems * 48, hipMemcpyDeviceToDevice, st));
  VO_HIP_CHECK(hipMemsetAsync(dout + r_sum, 0, (size_t)n_problems * 2 * sizeof(vo_lm_summary), st));
  VO_CHECK(vo_pose_only_solve_dev(n_problems, reinterpret_cast<const int32_t *>(di + o_off), 0,
                                  reinterpret_cast<const double *>(di + o_pts), reinterpret_cast<const double *>(di + o_obs),
                                  reinterpret_cast<const double *>(di + o_is), reinterpret_cast<const double *>(di + o_cam),
                                  reinterpret_cast<double *>(dout + r_pose), dout + r_out,
                                  reinterpret_cast<int32_t *>(dout + r_inl),
                                  reinterpret_cast<vo_lm_summary *>(dout + r_sum), st));
  // the inputs have left the staging block once the kernel has run: it takes the results back
  if (hipMemcpyAsync(stage, dout, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    vo::set_error("pose-only kernel failed: %s", hipGetErrorString(hipGetLastError()));
    return VO_ERR_HIP;
  }
  memcpy(poses, &stage[r_pose], (size_t)n_problems * 48);
  if (total > 0) memcpy(outlier, &stage[r_out], total);
  memcpy(n_inliers, &stage[r_inl], (size_t)n_problems * 4);
  if (summaries) memcpy(summaries, &stage[r_sum], (size_t)n_problems * 2 * sizeof(vo_lm_summary));
  return VO_OK;
}

}  // extern "C"
