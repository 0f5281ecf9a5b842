// sim3_horn.h -- one hypothesis of Sim3Solver::iterate (reference src/sim3Solver.cpp): Horn's closed form for three sampled
// correspondences (computeSim3 :179-240) and the projection of checkInliers (project :286-308), shared by k_sim3_ransac
// (loop.hip: vo_sim3_ransac_eval) and the walk over a store's loop candidates (loop_sim3.hip) so that both give the same bits.
// Include from translation units compiled with -ffp-contract=off only.
#pragma once
#include "triangulate.h"

namespace vo {

// Sim3Solver::computeSim3 (:179-252)
__device__ inline void sim3_horn(const double P1[9], const double P2[9], int fix_scale, double R[9], double t[3], double &s) {
  double O1[3] = {0, 0, 0}, O2[3] = {0, 0, 0}, Pr1[3][3], Pr2[3][3], M[3][3];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) O1[k] += P1[3 * i + k], O2[k] += P2[3 * i + k];
  for (int k = 0; k < 3; k++) O1[k] /= 3.0, O2[k] /= 3.0;
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) Pr1[k][i] = P1[3 * i + k] - O1[k], Pr2[k][i] = P2[3 * i + k] - O2[k];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      M[a][b] = 0;
      for (int i = 0; i < 3; i++) M[a][b] += Pr2[a][i] * Pr1[b][i];
    }
  double N[4][4], V[4][4], w[4];
  N[0][0] = M[0][0] + M[1][1] + M[2][2];
  N[0][1] = N[1][0] = M[1][2] - M[2][1];
  N[0][2] = N[2][0] = M[2][0] - M[0][2];
  N[0][3] = N[3][0] = M[0][1] - M[1][0];
  N[1][1] = M[0][0] - M[1][1] - M[2][2];
  N[1][2] = N[2][1] = M[0][1] + M[1][0];
  N[1][3] = N[3][1] = M[2][0] + M[0][2];
  N[2][2] = -M[0][0] + M[1][1] - M[2][2];
  N[2][3] = N[3][2] = M[1][2] + M[2][1];
  N[3][3] = -M[0][0] - M[1][1] + M[2][2];
  sym4_eigen(N, V, w);
  int best = 0;
  for (int i = 1; i < 4; i++)
    if (w[i] > w[best]) best = i;
  double q0 = V[0][best], q1 = V[1][best], q2 = V[2][best], q3 = V[3][best];  // (w, x, y, z)
  const double nq = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  q0 /= nq, q1 /= nq, q2 /= nq, q3 /= nq;
  R[0] = 1 - 2 * (q2 * q2 + q3 * q3), R[1] = 2 * (q1 * q2 - q0 * q3), R[2] = 2 * (q1 * q3 + q0 * q2);
  R[3] = 2 * (q1 * q2 + q0 * q3), R[4] = 1 - 2 * (q1 * q1 + q3 * q3), R[5] = 2 * (q2 * q3 - q0 * q1);
  R[6] = 2 * (q1 * q3 - q0 * q2), R[7] = 2 * (q2 * q3 + q0 * q1), R[8] = 1 - 2 * (q1 * q1 + q2 * q2);
  double sc = 1.0;
  if (!fix_scale) {
    double nom = 0, den = 0;
    for (int i = 0; i < 3; i++)
      for (int a = 0; a < 3; a++) {
        const double p3 = R[3 * a] * Pr2[0][i] + R[3 * a + 1] * Pr2[1][i] + R[3 * a + 2] * Pr2[2][i];
        nom += Pr1[a][i] * p3, den += p3 * p3;
      }
    sc = nom / den;
  }
  s = sc;
  for (int a = 0; a < 3; a++) t[a] = O1[a] - sc * (R[3 * a] * O2[0] + R[3 * a + 1] * O2[1] + R[3 * a + 2] * O2[2]);
}

__device__ __forceinline__ void sim3_project(const double *R, const double *t, double s, const double *p, float fx, float fy,
                                             float cx, float cy, double &u, double &v) {  // Sim3Solver::project :290-313
  const double x = s * (R[0] * p[0] + R[1] * p[1] + R[2] * p[2]) + t[0];
  const double y = s * (R[3] * p[0] + R[4] * p[1] + R[5] * p[2]) + t[1];
  const double z = s * (R[6] * p[0] + R[7] * p[1] + R[8] * p[2]) + t[2];
  const double invz = 1.0 / z;
  u = (double)((float)(x * invz) * fx + cx), v = (double)((float)(y * invz) * fy + cy);
}

// the inverse of (R, t, s) as Sophus::Sim3::inverse gives it: Ri = R^T, si = 1 / s, ti = -si Ri t.  T: R (9) t (3) s | Ri ti si
__device__ __forceinline__ void sim3_with_inverse(const double R[9], const double t[3], double s, double T[26]) {
  const double si = 1.0 / s;
  for (int a = 0; a < 9; a++) T[a] = R[a];
  for (int a = 0; a < 3; a++) T[9 + a] = t[a];
  T[12] = s;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) T[13 + 3 * a + b] = R[3 * b + a];
  for (int a = 0; a < 3; a++) T[22 + a] = -si * (T[13 + 3 * a] * t[0] + T[13 + 3 * a + 1] * t[1] + T[13 + 3 * a + 2] * t[2]);
  T[25] = si;
}

// checkInliers (:242-268) for correspondence i: both squared pixel errors against the integer thresholds
__device__ __forceinline__ bool sim3_inlier(const double T[26], const double *pc1, const double *pc2, const double *px1, const double *px2,
                                            int me1, int me2, float fx, float fy, float cx, float cy) {
  double u1, v1, u2, v2;
  sim3_project(T, T + 9, T[12], pc2, fx, fy, cx, cy, u1, v1);
  sim3_project(T + 13, T + 22, T[25], pc1, fx, fy, cx, cy, u2, v2);
  const double d1x = px1[0] - u1, d1y = px1[1] - v1, d2x = px2[0] - u2, d2y = px2[1] - v2;
  const float e1 = (float)(d1x * d1x + d1y * d1y), e2 = (float)(d2x * d2x + d2y * d2y);
  return e1 < (float)me1 && e2 < (float)me2;  // :260
}

}  // namespace vo
