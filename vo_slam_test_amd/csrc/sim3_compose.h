// sim3_compose.h -- the Sim3 algebra of the loop pose graph from the key-frame store, shared by the
// window's gather and the write-back (pose_graph_store.hip).  A Sim3 is 8 doubles as vo_sim3_reanchor_points takes them: the
// quaternion x y z w, the translation, the scale; S p = s * (R(q) p) + t.  Every operation is a double operation rounded on
// its own in the order written here (the file is compiled with -ffp-contract=off, and the pragma below says so again), so
// that tests/pose_graph_store_ref.py reproduces every result bit for bit.  The order is a choice of this restatement: Eigen
// and Sophus leave it to the compiler.
#pragma once
#include "vo_common.h"

#pragma clang fp contract(off)

namespace vo {

// (a * b + c * d) + e * f
__device__ __forceinline__ double s3_dot3(double a, double b, double c, double d, double e, double f) { return (a * b + c * d) + e * f; }

// q / |q|, |q| = sqrt(((x x + y y) + z z) + w w)
__device__ __forceinline__ void s3_normalize(double q[4]) {
  const double n = __dsqrt_rn(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int c = 0; c < 4; c++) q[c] = __ddiv_rn(q[c], n);
}

// Eigen's Quaternion(Matrix3) with its four branches; m row-major.  Not normalised.
__device__ __forceinline__ void s3_quat_from_matrix(const double *m, double q[4]) {
  double t = (m[0] + m[4]) + m[8];
  if (t > 0.0) {
    t = __dsqrt_rn(t + 1.0);
    q[3] = 0.5 * t;
    t = __ddiv_rn(0.5, t);
    q[0] = (m[7] - m[5]) * t, q[1] = (m[2] - m[6]) * t, q[2] = (m[3] - m[1]) * t;
    return;
  }
  int i = 0;
  if (m[4] > m[0]) i = 1;
  if (m[8] > m[4 * i]) i = 2;
  const int j = (i + 1) % 3, k = (j + 1) % 3;
  t = __dsqrt_rn(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
  q[i] = 0.5 * t;
  t = __ddiv_rn(0.5, t);
  q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
  q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
  q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
}

// Eigen's toRotationMatrix, R row-major
__device__ __forceinline__ void s3_matrix(const double *q, double R[9]) {
  const double tx = q[0] + q[0], ty = q[1] + q[1], tz = q[2] + q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

__device__ __forceinline__ void s3_rotate(const double *R, const double *p, double out[3]) {
  for (int r = 0; r < 3; r++) out[r] = s3_dot3(R[3 * r], p[0], R[3 * r + 1], p[1], R[3 * r + 2], p[2]);
}

// out = s * (R(q) p) + t
__device__ __forceinline__ void s3_act(const double *S, const double *p, double out[3]) {
  double R[9], r[3];
  s3_matrix(S, R);
  s3_rotate(R, p, r);
  for (int c = 0; c < 3; c++) out[c] = S[7] * r[c] + S[4 + c];
}

// out = A * B: q = normalised(qa qb) (Eigen's product), t = sa * (Ra tb) + ta, s = sa * sb.  out may not alias A or B.
__device__ __forceinline__ void s3_mul(const double *A, const double *B, double *out) {
  out[3] = ((A[3] * B[3] - A[0] * B[0]) - A[1] * B[1]) - A[2] * B[2];
  out[0] = ((A[3] * B[0] + A[0] * B[3]) + A[1] * B[2]) - A[2] * B[1];
  out[1] = ((A[3] * B[1] + A[1] * B[3]) + A[2] * B[0]) - A[0] * B[2];
  out[2] = ((A[3] * B[2] + A[2] * B[3]) + A[0] * B[1]) - A[1] * B[0];
  s3_normalize(out);
  s3_act(A, B + 4, out + 4);
  out[7] = A[7] * B[7];
}

// out = S^-1: q = conj(q), s = 1 / s, t = -(s' * (R(q') t)).  out may not alias S.
__device__ __forceinline__ void s3_inv(const double *S, double *out) {
  out[0] = -S[0], out[1] = -S[1], out[2] = -S[2], out[3] = S[3];
  out[7] = __ddiv_rn(1.0, S[7]);
  double R[9], r[3];
  s3_matrix(out, R);
  s3_rotate(R, S + 4, r);
  for (int c = 0; c < 3; c++) out[4 + c] = -(out[7] * r[c]);
}

// a Sim3 as an entry point received it: the quaternion normalised, the rest as given
__device__ __forceinline__ void s3_load(const double *src, double *S) {
  for (int c = 0; c < 8; c++) S[c] = src[c];
  s3_normalize(S);
}

// (unit_quaternion(R) normalised, t, 1) of a pose column entry Tcw12 = R row-major, t
__device__ __forceinline__ void s3_from_pose(const double *T, double *S) {
  s3_quat_from_matrix(T, S);
  s3_normalize(S);
  S[4] = T[9], S[5] = T[10], S[6] = T[11], S[7] = 1.0;
}

}  // namespace vo
