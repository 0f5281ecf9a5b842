// handover_geom.h -- the pose arithmetic of the hand-over (handover.hip): Tcl_ = Tcw * Tlw^-1
// (visualOdometry.cpp:96) and frame_curr_->setPose(Tcl_ * frame_last_->Tcw_) (:236) on poses held as R row-major (9) then t (3).
// Every operation is an explicitly rounded double operation in the order written here, so that tests/handover_ref.py
// reproduces VELOCITY and the start Tcw bit for bit from the FRAME_POSE the device reports.  (Sophus composes unit quaternions
// and renormalises; that rounding is not reproduced, as in keyframe_geom.h.)  The temporary points' back-projection is
// keyframe_geom.h's kc_pixel2camera and kc_camera2world.
#pragma once
#include "ba_math.h"
#include "keyframe_geom.h"

namespace vo {

// R, t of a pose given as unit quaternion (w, x, y, z) + translation: the arithmetic of vo_se3_exp (vo_common.hip) behind
// se3_exp -- tx = 2 x, twx = tx w, txx = tx x, ...; R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy, ...
__device__ __forceinline__ void ho_pose12(const ba::Se3 &P, double T[12]) {
  const double *q = P.q;
  const double tx = __dmul_rn(2.0, q[1]), ty = __dmul_rn(2.0, q[2]), tz = __dmul_rn(2.0, q[3]);
  const double twx = __dmul_rn(tx, q[0]), twy = __dmul_rn(ty, q[0]), twz = __dmul_rn(tz, q[0]);
  const double txx = __dmul_rn(tx, q[1]), txy = __dmul_rn(ty, q[1]), txz = __dmul_rn(tz, q[1]);
  const double tyy = __dmul_rn(ty, q[2]), tyz = __dmul_rn(tz, q[2]), tzz = __dmul_rn(tz, q[3]);
  T[0] = __dsub_rn(1.0, __dadd_rn(tyy, tzz)), T[1] = __dsub_rn(txy, twz), T[2] = __dadd_rn(txz, twy);
  T[3] = __dadd_rn(txy, twz), T[4] = __dsub_rn(1.0, __dadd_rn(txx, tzz)), T[5] = __dsub_rn(tyz, twx);
  T[6] = __dsub_rn(txz, twy), T[7] = __dadd_rn(tyz, twx), T[8] = __dsub_rn(1.0, __dadd_rn(txx, tyy));
  T[9] = P.t[0], T[10] = P.t[1], T[11] = P.t[2];
}

// T^-1: R^T, and t' = -(R^T t) = np_center: t'[i] = -((R[0][i] t[0] + R[1][i] t[1]) + R[2][i] t[2])
__device__ __forceinline__ void ho_inverse(const double *T, double out[12]) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) out[3 * i + j] = T[3 * j + i];
  np_center(T, out + 9);
}

// A * B: R[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j];
// t[i] = ((A[i][0] tB[0] + A[i][1] tB[1]) + A[i][2] tB[2]) + tA[i]
__device__ __forceinline__ void ho_compose(const double *A, const double *B, double out[12]) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) out[3 * i + j] = np_dot3(A[3 * i], B[j], A[3 * i + 1], B[3 + j], A[3 * i + 2], B[6 + j]);
    out[9 + i] = __dadd_rn(np_dot3(A[3 * i], B[9], A[3 * i + 1], B[10], A[3 * i + 2], B[11]), A[9 + i]);
  }
}

}  // namespace vo
