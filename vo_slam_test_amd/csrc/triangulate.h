// triangulate.h -- the 4 x 4 linear triangulation of LocalMapping::createNewMapPoints (src/localMapping.cpp:234-251) and the
// symmetric eigen-decomposition behind it, shared by k_triangulate (loop.hip: vo_triangulate) and k_np_create
// (new_points.hip: vo_kfstore_create_map_points) so that both give the same bits.  Include from translation units
// compiled with -ffp-contract=off only.
#pragma once
#include <hip/hip_runtime.h>

namespace vo {

// symmetric 4 x 4 eigen-decomposition, cyclic Jacobi (Eigen::EigenSolver of a symmetric matrix / cv::SVD of a 4 x 4:
// same vectors up to sign and rounding)
__device__ inline void sym4_eigen(double A[4][4], double V[4][4], double w[4]) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) V[i][j] = i == j;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0;
    for (int p = 0; p < 4; p++)
      for (int q = p + 1; q < 4; q++) off += A[p][q] * A[p][q];
    if (off < 1e-300) break;
    for (int p = 0; p < 4; p++)
      for (int q = p + 1; q < 4; q++) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; k++) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; k++) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 4; i++) w[i] = A[i][i];
}

// one pair: normalised image points (x1, y1), (x2, y2), poses T1, T2 (3 x 4 row-major, float as the reference's cv::Mat) ->
// out [3]; false (out = 0) when the null vector has |x3| < 1e-8 (:245-246)
__device__ inline bool triangulate_pair(float x1, float y1, float x2, float y2, const float *T1, const float *T2, float out[3]) {
  float A[4][4];
  for (int c = 0; c < 4; c++) {
    A[0][c] = x1 * T1[8 + c] - T1[c];
    A[1][c] = y1 * T1[8 + c] - T1[4 + c];
    A[2][c] = x2 * T2[8 + c] - T2[c];
    A[3][c] = y2 * T2[8 + c] - T2[4 + c];
  }
  double G[4][4], V[4][4], w[4];
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++) {
      G[a][b] = 0;
      for (int r = 0; r < 4; r++) G[a][b] += (double)A[r][a] * (double)A[r][b];
    }
  sym4_eigen(G, V, w);
  int best = 0;
  for (int q = 1; q < 4; q++)
    if (w[q] < w[best]) best = q;
  const float x3 = (float)V[3][best];
  const bool good = !(fabsf(x3) < 1e-8f);  // :245-246
  for (int a = 0; a < 3; a++) out[a] = good ? (float)V[a][best] / x3 : 0.f;
  return good;
}

}  // namespace vo
