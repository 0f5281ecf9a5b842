// pnp.hip -- cv::solvePnPRansac(pts3d, pts2d, K, noArray(), rvec, tvec, false, iters, err, conf, inliers, SOLVEPNP_EPNP)
// as VisualOdometry::poseEstimateByPnP calls it (reference src/visualOdometry.cpp:778-830), restated from the published
// EPnP (Lepetit et al. 2009) and OpenCV 3.x's ptsetreg.cpp / solvepnp.cpp / epnp.cpp conventions, for a
// ragged batch of problems (problem p owns correspondences offsets[p] .. offsets[p+1]).  Four launches, no host sync:
//   k_pnp_samples   cv::RNG((uint64)-1) + getSubset, one lane per problem: the 5-tuples of every iteration
//   k_pnp_epnp      EPnP in FP64 on a 16-lane group: one group per (problem, hypothesis), or per problem for the refit
//                   over the winner's inliers.  M^T M (12 x 12) lives in LDS by elements, its eigen-decomposition is a
//                   parallel-ordered (round-robin) cyclic Jacobi: 6 disjoint rotations per round, 9 + 9 elements of A and
//                   V per lane; the rest of EPnP (L_6x10, rho, three beta approximations, Gauss-Newton, R and t) runs
//                   redundantly in every lane of the group (no exchange needed)
//   k_pnp_score     a workgroup per problem, correspondences staged in LDS: one wave per hypothesis at a time, ballot +
//                   popcount per 64 correspondences -> inlier count per hypothesis
//   k_pnp_replay    one lane per problem: the ordered RANSAC loop over the counts (RANSACUpdateNumIters), then the
//                   winner's inlier mask (recomputed with the scoring code)
// Compiled with -ffp-contract=off (the float reprojection gate must round like the x86-64 reference build).
#include "vo_common.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kModel = 5;        // model_points of the EPnP kernel
constexpr int kGroup = 16;       // lanes per EPnP solve
constexpr int kEpnpBlock = 64;   // 4 solves per workgroup
constexpr int kStage = 2048;     // correspondences staged in LDS per scoring chunk
constexpr int kMaxSweeps = 16;   // Jacobi sweeps (12 x 12 converges in 6-9)

struct Cam {
  double fu, fv, uc, vc;
};

// ---------------------------------------------------------------------------------------------------------------- small
__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// symmetric 3 x 3 eigen-decomposition, cyclic Jacobi; eigenvalues descending, vectors as rows of U with their largest-
// magnitude component positive (cvSVD's U^T of a symmetric PSD matrix up to the sign, which is fixed here)
__device__ void sym3_eigen_desc(double A[3][3], double w[3], double U[3][3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 30; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    if (off == 0.0) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; k++) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int o[3] = {0, 1, 2};
  for (int i = 0; i < 3; i++)
    for (int j = i + 1; j < 3; j++)
      if (A[o[j]][o[j]] > A[o[i]][o[i]]) {
        const int x = o[i];
        o[i] = o[j], o[j] = x;
      }
  for (int i = 0; i < 3; i++) {
    w[i] = A[o[i]][o[i]];
    int m = 0;
    for (int k = 1; k < 3; k++)
      if (fabs(V[k][o[i]]) > fabs(V[m][o[i]])) m = k;
    const double sg = V[m][o[i]] < 0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; k++) U[i][k] = sg * V[k][o[i]];
  }
}

// epnp.cpp qr_solve: Householder QR least squares of an nr x nc system (nr <= 6, nc <= 5), A and b overwritten
template <int NR, int NC>
__device__ void qr_solve(double A[NR][NC], double b[NR], double X[NC]) {
  double A1[NC], A2[NC];
  for (int k = 0; k < NC; k++) X[k] = 0.0;
  for (int k = 0; k < NC; k++) {
    double eta = fabs(A[k][k]);
    for (int i = k + 1; i < NR; i++) eta = fmax(eta, fabs(A[i][k]));
    if (eta == 0) return;  // singular: X stays 0 (epnp.cpp leaves it unset)
    double sum2 = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < NR; i++) {
      A[i][k] *= inv_eta;
      sum2 += A[i][k] * A[i][k];
    }
    double sigma = sqrt(sum2);
    if (A[k][k] < 0) sigma = -sigma;
    A[k][k] += sigma;
    A1[k] = sigma * A[k][k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < NC; j++) {
      double sum = 0;
      for (int i = k; i < NR; i++) sum += A[i][k] * A[i][j];
      const double tau = sum / A1[k];
      for (int i = k; i < NR; i++) A[i][j] -= tau * A[i][k];
    }
  }
  for (int j = 0; j < NC; j++) {
    double tau = 0;
    for (int i = j; i < NR; i++) tau += A[i][j] * b[i];
    tau /= A1[j];
    for (int i = j; i < NR; i++) b[i] -= tau * A[i][j];
  }
  X[NC - 1] = b[NC - 1] / A2[NC - 1];
  for (int i = NC - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < NC; j++) sum += A[i][j] * X[j];
    X[i] = (b[i] - sum) / A2[i];
  }
}

// The point set of one solve: a 5-tuple of sample indices, or every correspondence of a problem whose mask bit is set.
struct PtSet {
  const float *p3, *p2;  // the problem's correspondences
  const int *idx;        // [5] sample indices, or NULL
  const uint8_t *mask;   // [n] or NULL (all)
  int n;                 // 5 with idx, else the problem's size
  __device__ __forceinline__ bool get(int k, double pw[3], double u[2]) const {
    if (mask && !mask[k]) return false;
    const int i = idx ? idx[k] : k;
    pw[0] = p3[3 * i], pw[1] = p3[3 * i + 1], pw[2] = p3[3 * i + 2];
    u[0] = p2[2 * i], u[1] = p2[2 * i + 1];
    return true;
  }
};

struct EpnpShared {
  double A[144], V[144];  // M^T M (row-major) and the accumulated rotations
  double cs[6][2];
};

// the round-robin pairs of round r (0..10) of a 12-index cyclic Jacobi: (r, 11) and ((r+k)%11, (r-k)%11), k = 1..5
__device__ __forceinline__ void rr_pair(int r, int k, int &p, int &q) {
  int a, b;
  if (k == 0)
    a = r, b = 11;
  else
    a = (r + k) % 11, b = (r + 11 - k) % 11;
  p = a < b ? a : b, q = a < b ? b : a;
}
__device__ __forceinline__ void rr_role(int r, int i, int &k, int &partner, bool &first) {  // index i's pair in round r
  if (i == 11 || i == r) {
    k = 0, partner = i == 11 ? r : 11;
  } else {
    const int d = (i - r + 11) % 11;  // i = r + d or r - (11 - d)
    k = d <= 5 ? d : 11 - d;
    partner = d <= 5 ? (r + 11 - k) % 11 : (r + k) % 11;
  }
  first = i < partner;
}

// compute_R_and_t of epnp.cpp for one set of betas: ccs, pcs (sign fix on the first point), Procrustes, mean reprojection
// error over the set.  R's orthogonal polar factor by scaled Newton iteration (= U V^T of cvSVD), det < 0 -> row 2 negated.
__device__ double compute_R_and_t(const PtSet &S, int cnt, const double cws[4][3], const double ci[9], const double v[4][12],
                                  const double betas[4], const Cam &cam, double R[3][3], double t[3]) {
  double ccs[4][3];
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 3; k++) ccs[j][k] = 0.0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[i][3 * j + k];
  // pcs are recomputed from the alphas where needed (not stored): pc = sum_j a_j ccs_j
  auto alphas = [&](const double pw[3], double a[4]) {
    const double d0 = pw[0] - cws[0][0], d1 = pw[1] - cws[0][1], d2 = pw[2] - cws[0][2];
    for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
  };
  auto pc_of = [&](const double a[4], double pc[3]) {
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
  };
  double sgn = 1.0;  // solve_for_sign: the first point of the set behind the camera -> every pc negated
  for (int k = 0; k < S.n; k++) {
    double pw[3], u[2], a[4], pc[3];
    if (!S.get(k, pw, u)) continue;
    alphas(pw, a);
    pc_of(a, pc);
    if (pc[2] < 0.0) sgn = -1.0;
    break;
  }
  double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
  for (int k = 0; k < S.n; k++) {
    double pw[3], u[2], a[4], pc[3];
    if (!S.get(k, pw, u)) continue;
    alphas(pw, a);
    pc_of(a, pc);
    for (int j = 0; j < 3; j++) pc0[j] += sgn * pc[j], pw0[j] += pw[j];
  }
  for (int j = 0; j < 3; j++) pc0[j] /= cnt, pw0[j] /= cnt;
  double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int k = 0; k < S.n; k++) {
    double pw[3], u[2], a[4], pc[3];
    if (!S.get(k, pw, u)) continue;
    alphas(pw, a);
    pc_of(a, pc);
    for (int j = 0; j < 3; j++) {
      const double dc = sgn * pc[j] - pc0[j];
      H[j][0] += dc * (pw[0] - pw0[0]);
      H[j][1] += dc * (pw[1] - pw0[1]);
      H[j][2] += dc * (pw[2] - pw0[2]);
    }
  }
  // polar factor: X <- (g X + X^-T / g) / 2, g = sqrt(|X^-1|_F / |X|_F)
  double X[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) X[a][b] = H[a][b];
  for (int it = 0; it < 40; it++) {
    double C[3][3];  // cofactors: X^-T = C / det
    C[0][0] = X[1][1] * X[2][2] - X[1][2] * X[2][1];
    C[0][1] = X[1][2] * X[2][0] - X[1][0] * X[2][2];
    C[0][2] = X[1][0] * X[2][1] - X[1][1] * X[2][0];
    C[1][0] = X[0][2] * X[2][1] - X[0][1] * X[2][2];
    C[1][1] = X[0][0] * X[2][2] - X[0][2] * X[2][0];
    C[1][2] = X[0][1] * X[2][0] - X[0][0] * X[2][1];
    C[2][0] = X[0][1] * X[1][2] - X[0][2] * X[1][1];
    C[2][1] = X[0][2] * X[1][0] - X[0][0] * X[1][2];
    C[2][2] = X[0][0] * X[1][1] - X[0][1] * X[1][0];
    const double det = X[0][0] * C[0][0] + X[0][1] * C[0][1] + X[0][2] * C[0][2];
    if (det == 0.0 || !isfinite(det)) break;
    double nx = 0, ni = 0;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) nx += X[a][b] * X[a][b], ni += C[a][b] * C[a][b];
    const double g = sqrt(sqrt(ni) / fabs(det) / sqrt(nx));
    double diff = 0;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        const double y = 0.5 * (g * X[a][b] + C[a][b] / (g * det));
        diff += (y - X[a][b]) * (y - X[a][b]);
        X[a][b] = y;
      }
    if (diff < 1e-30) break;
  }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) R[a][b] = X[a][b];
  const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                     R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
  if (det < 0) R[2][0] = -R[2][0], R[2][1] = -R[2][1], R[2][2] = -R[2][2];
  t[0] = pc0[0] - dot3(R[0], pw0);
  t[1] = pc0[1] - dot3(R[1], pw0);
  t[2] = pc0[2] - dot3(R[2], pw0);
  double sum2 = 0.0;  // reprojection_error
  for (int k = 0; k < S.n; k++) {
    double pw[3], u[2];
    if (!S.get(k, pw, u)) continue;
    const double Xc = dot3(R[0], pw) + t[0], Yc = dot3(R[1], pw) + t[1];
    const double inv_Zc = 1.0 / (dot3(R[2], pw) + t[2]);
    const double ue = cam.uc + cam.fu * Xc * inv_Zc, ve = cam.vc + cam.fv * Yc * inv_Zc;
    sum2 += sqrt((u[0] - ue) * (u[0] - ue) + (u[1] - ve) * (u[1] - ve));
  }
  return sum2 / cnt;
}

__device__ void gauss_newton(const double L[6][10], const double rho[6], double betas[4]) {
  for (int it = 0; it < 5; it++) {
    double A[6][4], b[6], x[4];
    for (int i = 0; i < 6; i++) {
      const double *l = L[i];
      A[i][0] = 2 * l[0] * betas[0] + l[1] * betas[1] + l[3] * betas[2] + l[6] * betas[3];
      A[i][1] = l[1] * betas[0] + 2 * l[2] * betas[1] + l[4] * betas[2] + l[7] * betas[3];
      A[i][2] = l[3] * betas[0] + l[4] * betas[1] + 2 * l[5] * betas[2] + l[8] * betas[3];
      A[i][3] = l[6] * betas[0] + l[7] * betas[1] + l[8] * betas[2] + 2 * l[9] * betas[3];
      b[i] = rho[i] - (l[0] * betas[0] * betas[0] + l[1] * betas[0] * betas[1] + l[2] * betas[1] * betas[1] +
                       l[3] * betas[0] * betas[2] + l[4] * betas[1] * betas[2] + l[5] * betas[2] * betas[2] +
                       l[6] * betas[0] * betas[3] + l[7] * betas[1] * betas[3] + l[8] * betas[2] * betas[3] +
                       l[9] * betas[3] * betas[3]);
    }
    qr_solve<6, 4>(A, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

// One EPnP solve (epnp::compute_pose) by a 16-lane group.  Every lane of the workgroup calls it (the barriers are block-
// wide); `active` = 0 for a group without work (it still takes part in the barriers).  Output R (row-major), t in every
// lane of the group.
__device__ void epnp_group(const PtSet &S, bool active, EpnpShared &sh, int lane, const Cam &cam, double Rout[9], double tout[3]) {
  // the set's size and control points (choose_control_points): redundant in every lane, no exchange
  int cnt = 0;
  double cws[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (active)
    for (int k = 0; k < S.n; k++) {
      double pw[3], u[2];
      if (!S.get(k, pw, u)) continue;
      cnt++;
      for (int j = 0; j < 3; j++) cws[0][j] += pw[j];
    }
  const double inv_n = 1.0 / (cnt > 0 ? cnt : 1);
  for (int j = 0; j < 3; j++) cws[0][j] = cnt > 0 ? cws[0][j] / cnt : 0.0;
  double P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (active)
    for (int k = 0; k < S.n; k++) {
      double pw[3], u[2];
      if (!S.get(k, pw, u)) continue;
      const double d[3] = {pw[0] - cws[0][0], pw[1] - cws[0][1], pw[2] - cws[0][2]};
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) P[a][b] += d[a] * d[b];
    }
  double dc[3], uct[3][3];
  sym3_eigen_desc(P, dc, uct);
  for (int i = 1; i < 4; i++) {
    const double k = sqrt(fmax(dc[i - 1], 0.0) * inv_n);  // (a rounding-negative eigenvalue of a PSD matrix: 0)
    for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * uct[i - 1][j];
  }
  // barycentric coordinates: CC^-1 as cvInvert(CV_SVD) forms it.  CC's columns are k_j u_j (orthonormal u_j), so its SVD
  // is known: CC^+ = diag(1 / k) U^T, a singular value <= 2 DBL_EPSILON (k_1 + k_2 + k_3) dropped (SVBkSb's threshold) --
  // coplanar, collinear or coincident points give finite coordinates, not an overflowing adjugate
  double ci[9];
  {
    double k[3];
    for (int j = 0; j < 3; j++) k[j] = sqrt(fmax(dc[j], 0.0) * inv_n);
    const double thr = 2.0 * 2.220446049250313e-16 * (k[0] + k[1] + k[2]);
    for (int j = 0; j < 3; j++) {
      const double ik = k[j] > thr ? 1.0 / k[j] : 0.0;
      for (int c = 0; c < 3; c++) ci[3 * j + c] = uct[j][c] * ik;
    }
  }
  // M^T M by elements: lane l owns the upper-triangle entries l, l + 16, .. of 78 and sums them over the set's rows
  for (int e = lane; e < 78; e += kGroup) {
    int a = 0, rem = e;
    while (rem >= 12 - a) rem -= 12 - a, a++;
    const int b = a + rem;
    const int ja = a / 3, ca = a % 3, jb = b / 3, cb = b % 3;
    double s = 0.0;
    if (active)
      for (int k = 0; k < S.n; k++) {
        double pw[3], u[2];
        if (!S.get(k, pw, u)) continue;
        const double d0 = pw[0] - cws[0][0], d1 = pw[1] - cws[0][1], d2 = pw[2] - cws[0][2];
        double al[4];
        for (int j = 0; j < 3; j++) al[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
        al[0] = 1.0 - al[1] - al[2] - al[3];
        // row 1: (a fu, 0, a (uc - u)), row 2: (0, a fv, a (vc - v)) per control point
        const double m1a = ca == 0 ? al[ja] * cam.fu : ca == 1 ? 0.0 : al[ja] * (cam.uc - u[0]);
        const double m1b = cb == 0 ? al[jb] * cam.fu : cb == 1 ? 0.0 : al[jb] * (cam.uc - u[0]);
        const double m2a = ca == 0 ? 0.0 : ca == 1 ? al[ja] * cam.fv : al[ja] * (cam.vc - u[1]);
        const double m2b = cb == 0 ? 0.0 : cb == 1 ? al[jb] * cam.fv : al[jb] * (cam.vc - u[1]);
        s += m1a * m1b;
        s += m2a * m2b;
      }
    sh.A[12 * a + b] = s;
    sh.A[12 * b + a] = s;
  }
  for (int e = lane; e < 144; e += kGroup) sh.V[e] = (e / 12 == e % 12) ? 1.0 : 0.0;
  __syncthreads();
  // parallel-ordered cyclic Jacobi: per round 6 disjoint rotations (lanes 0..5 compute the angles), then each lane
  // rewrites 9 elements of A (A' = J^T A J, columns then rows) and 9 of V (V' = V J).  A group stops rotating at the
  // first sweep whose convergence test it passes and leaves A and V untouched from then on, while it keeps reaching the
  // barriers until every group of the workgroup is done: a solve's bits do not depend on which solves share its
  // workgroup (its position in the batch, its neighbours' convergence)
  bool done = !active;
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    // convergence: off-diagonal mass below 1e-30 of the diagonal's (the butterfly gives every lane the same sums)
    double off = 0, dg = 0;
    for (int e = lane; e < 144; e += kGroup) {
      const double x = sh.A[e] * sh.A[e];
      if (e / 12 == e % 12)
        dg += x;
      else
        off += x;
    }
    for (int o = kGroup / 2; o >= 1; o >>= 1) off += __shfl_xor(off, o, kGroup), dg += __shfl_xor(dg, o, kGroup);
    done = done || !(off > 1e-30 * dg);
    if (!__syncthreads_or(!done)) break;
    for (int r = 0; r < 11; r++) {
      if (lane < 6) {
        int p, q;
        rr_pair(r, lane, p, q);
        const double apq = sh.A[12 * p + q];
        double c = 1.0, s = 0.0;
        if (apq != 0.0) {
          const double theta = (sh.A[12 * q + q] - sh.A[12 * p + p]) / (2.0 * apq);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        }
        sh.cs[lane][0] = c, sh.cs[lane][1] = s;
      }
      __syncthreads();
      double na[9], nv[9];
      for (int m = 0; m < 9; m++) {
        const int e = lane + kGroup * m, i = e / 12, j = e % 12;
        int ki, pi, kj, pj;
        bool fi, fj;
        rr_role(r, i, ki, pi, fi);
        rr_role(r, j, kj, pj, fj);
        const double ci_ = sh.cs[ki][0], si = sh.cs[ki][1], cj = sh.cs[kj][0], sj = sh.cs[kj][1];
        // B[x][j] = (A J)[x][j]: j first of its pair: c A[x][j] - s A[x][pj]; second: s A[x][pj] + c A[x][j]
        auto colrot = [&](int x) {
          return fj ? cj * sh.A[12 * x + j] - sj * sh.A[12 * x + pj] : sj * sh.A[12 * x + pj] + cj * sh.A[12 * x + j];
        };
        const double bi = colrot(i), bp = colrot(pi);
        na[m] = fi ? ci_ * bi - si * bp : si * bp + ci_ * bi;
        nv[m] = fj ? cj * sh.V[12 * i + j] - sj * sh.V[12 * i + pj] : sj * sh.V[12 * i + pj] + cj * sh.V[12 * i + j];
      }
      __syncthreads();
      if (!done)  // (only the write-back is guarded: a guard on the loops above costs the kernel scratch)
        for (int m = 0; m < 9; m++) sh.A[lane + kGroup * m] = na[m], sh.V[lane + kGroup * m] = nv[m];
      __syncthreads();
    }
  }
  // the 4 smallest eigenvalues ascending (ties: lower index): v[0] = ut row 11 of epnp.cpp, .. v[3] = row 8
  double v[4][12];
  {
    int taken = 0;
    for (int i = 0; i < 4; i++) {
      int best = -1;
      for (int k = 0; k < 12; k++)
        if (!((taken >> k) & 1) && (best < 0 || sh.A[13 * k] < sh.A[13 * best])) best = k;
      taken |= 1 << best;
      for (int k = 0; k < 12; k++) v[i][k] = sh.V[12 * k + best];
    }
  }
  // five points: M (10 x 12) has a two-dimensional null space whose basis the solver picks by rounding; fixed here by
  // rotating it so that v[1][0] = 0, v[0][0] >= 0
  if (cnt == kModel) {
    const double g = sqrt(v[0][0] * v[0][0] + v[1][0] * v[1][0]);
    if (g > 0) {
      const double c = v[0][0] / g, s = v[1][0] / g;
      for (int k = 0; k < 12; k++) {
        const double a = v[0][k], b = v[1][k];
        v[0][k] = c * a + s * b, v[1][k] = c * b - s * a;
      }
      v[1][0] = 0.0;
    }
  }
  // compute_L_6x10, compute_rho
  double L[6][10], rho[6];
  {
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
      int a = 0, b = 1;
      for (int j = 0; j < 6; j++) {
        for (int k = 0; k < 3; k++) dv[i][j][k] = v[i][3 * a + k] - v[i][3 * b + k];
        b++;
        if (b > 3) a++, b = a + 1;
      }
    }
    for (int i = 0; i < 6; i++) {
      L[i][0] = dot3(dv[0][i], dv[0][i]);
      L[i][1] = 2.0 * dot3(dv[0][i], dv[1][i]);
      L[i][2] = dot3(dv[1][i], dv[1][i]);
      L[i][3] = 2.0 * dot3(dv[0][i], dv[2][i]);
      L[i][4] = 2.0 * dot3(dv[1][i], dv[2][i]);
      L[i][5] = dot3(dv[2][i], dv[2][i]);
      L[i][6] = 2.0 * dot3(dv[0][i], dv[3][i]);
      L[i][7] = 2.0 * dot3(dv[1][i], dv[3][i]);
      L[i][8] = 2.0 * dot3(dv[2][i], dv[3][i]);
      L[i][9] = dot3(dv[3][i], dv[3][i]);
    }
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
      const double d[3] = {cws[a][0] - cws[b][0], cws[a][1] - cws[b][1], cws[a][2] - cws[b][2]};
      rho[j] = dot3(d, d);
      b++;
      if (b > 3) a++, b = a + 1;
    }
  }
  double bestR[3][3], bestT[3], bestErr = 0;
  for (int N = 1; N <= 3; N++) {
    double betas[4];
    if (N == 1) {  // [B11 B12 B13 B14]
      double A[6][4], b[6], x[4];
      for (int i = 0; i < 6; i++) A[i][0] = L[i][0], A[i][1] = L[i][1], A[i][2] = L[i][3], A[i][3] = L[i][6], b[i] = rho[i];
      qr_solve<6, 4>(A, b, x);
      if (x[0] < 0) {
        betas[0] = sqrt(-x[0]);
        betas[1] = -x[1] / betas[0], betas[2] = -x[2] / betas[0], betas[3] = -x[3] / betas[0];
      } else {
        betas[0] = sqrt(x[0]);
        betas[1] = x[1] / betas[0], betas[2] = x[2] / betas[0], betas[3] = x[3] / betas[0];
      }
    } else if (N == 2) {  // [B11 B12 B22]
      double A[6][3], b[6], x[3];
      for (int i = 0; i < 6; i++) A[i][0] = L[i][0], A[i][1] = L[i][1], A[i][2] = L[i][2], b[i] = rho[i];
      qr_solve<6, 3>(A, b, x);
      if (x[0] < 0) {
        betas[0] = sqrt(-x[0]);
        betas[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
      } else {
        betas[0] = sqrt(x[0]);
        betas[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
      }
      if (x[1] < 0) betas[0] = -betas[0];
      betas[2] = 0.0, betas[3] = 0.0;
    } else {  // [B11 B12 B22 B13 B23]
      double A[6][5], b[6], x[5];
      for (int i = 0; i < 6; i++)
        A[i][0] = L[i][0], A[i][1] = L[i][1], A[i][2] = L[i][2], A[i][3] = L[i][3], A[i][4] = L[i][4], b[i] = rho[i];
      qr_solve<6, 5>(A, b, x);
      if (x[0] < 0) {
        betas[0] = sqrt(-x[0]);
        betas[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
      } else {
        betas[0] = sqrt(x[0]);
        betas[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
      }
      if (x[1] < 0) betas[0] = -betas[0];
      betas[2] = x[3] / betas[0];
      betas[3] = 0.0;
    }
    gauss_newton(L, rho, betas);
    double R[3][3], t[3];
    const double err = active ? compute_R_and_t(S, cnt, cws, ci, v, betas, cam, R, t) : 0.0;
    if (N == 1 || err < bestErr) {
      bestErr = err;
      for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) bestR[a][b] = R[a][b];
        bestT[a] = t[a];
      }
    }
  }
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) Rout[3 * a + b] = bestR[a][b];
    tout[a] = bestT[a];
  }
}

// ---------------------------------------------------------------------------------------------------------------- kernels
// cv::RNG((uint64)-1): state = (uint64)(uint32)state * 4164903690 + (state >> 32); getSubset redraws a repeated index
__global__ __launch_bounds__(64) void k_pnp_samples(int P, const int *offsets, int iters, int *samples) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int n = offsets[p + 1] - offsets[p];
  if (n <= kModel) return;
  uint64_t st = ~0ull;
  int *out = samples + (size_t)p * iters * kModel;
  for (int it = 0; it < iters; it++) {
    int idx[kModel];
    for (int i = 0; i < kModel; i++) {
      for (;;) {
        st = (uint64_t)(uint32_t)st * 4164903690u + (st >> 32);
        const int c = (int)((uint32_t)st % (uint32_t)n);
        int j = 0;
        while (j < i && idx[j] != c) j++;
        if (j == i) {
          idx[i] = c;
          break;
        }
      }
      out[it * kModel + i] = idx[i];
    }
  }
}

// mode 0: one group per (problem, iteration) -> hyp [P][iters][12]; mode 1: one group per problem over its mask (the
// refit, problems with status 1) -> Tcw [P][12]
// mode 0: one group per (problem, iteration) -> hyp [P][iters][12]; mode 1: one group per problem over its mask (the
// refit, problems with status 1) -> Tcw [P][12]; a refit that is not finite fails the problem (status 0, mask cleared)
__global__ __launch_bounds__(kEpnpBlock) void k_pnp_epnp(int mode, int P, int iters, const int *offsets, const float *pts3d,
                                                         const float *pts2d, Cam cam, const int *samples, uint8_t *mask,
                                                         int *status, int *n_inl, double *out) {
  __shared__ EpnpShared sh[kEpnpBlock / kGroup];
  const int g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
  const long job = (long)blockIdx.x * (kEpnpBlock / kGroup) + g;
  const long n_jobs = mode == 0 ? (long)P * iters : P;
  const int p = (int)(job < n_jobs ? (mode == 0 ? job / iters : job) : 0);
  const int o0 = offsets[p], n = offsets[p + 1] - o0;
  bool active = job < n_jobs;
  PtSet S;
  S.p3 = pts3d + 3 * (size_t)o0, S.p2 = pts2d + 2 * (size_t)o0;
  int idx[kModel];
  if (mode == 0) {
    active = active && n > kModel;
    if (active)
      for (int i = 0; i < kModel; i++) idx[i] = samples[job * kModel + i];
    S.idx = idx, S.mask = nullptr, S.n = kModel;
  } else {
    active = active && status[p] == 1;
    S.idx = nullptr, S.mask = mask + o0, S.n = n;
  }
  double R[9], t[3];
  epnp_group(S, active, sh[g], lane, cam, R, t);  // (its barriers separate the reads of status / mask above from the writes)
  if (!active) return;
  bool finite = true;
  for (int a = 0; a < 9; a++) finite = finite && isfinite(R[a]);
  for (int a = 0; a < 3; a++) finite = finite && isfinite(t[a]);
  if (mode == 1 && !finite) {
    for (int i = lane; i < n; i += kGroup) mask[o0 + i] = 0;
    if (lane == 0) status[p] = 0, n_inl[p] = 0;
    return;
  }
  if (lane == 0) {
    double *o = out + 12 * job;
    for (int a = 0; a < 3; a++) {
      o[4 * a] = R[3 * a], o[4 * a + 1] = R[3 * a + 1], o[4 * a + 2] = R[3 * a + 2];
      o[4 * a + 3] = t[a];
    }
  }
}

// computeError of the PnP callback: projectPoints in double (no distortion), the projection stored as float, squared
// distance in float; inlier when <= (float)(thresh * thresh)
__device__ __forceinline__ bool pnp_inlier(const double *T, float X, float Y, float Z, float u, float v, const Cam &cam, float th2) {
  const double Xd = X, Yd = Y, Zd = Z;
  double x = T[0] * Xd + T[1] * Yd + T[2] * Zd + T[3];
  double y = T[4] * Xd + T[5] * Yd + T[6] * Zd + T[7];
  double z = T[8] * Xd + T[9] * Yd + T[10] * Zd + T[11];
  z = z != 0.0 ? 1. / z : 1;
  x *= z, y *= z;
  const float pu = (float)(x * cam.fu + cam.uc), pv = (float)(y * cam.fv + cam.vc);
  const float dx = u - pu, dy = v - pv;
  const float err = dx * dx + dy * dy;
  return err <= th2;
}

__global__ __launch_bounds__(256) void k_pnp_score(int iters, const int *offsets, const float *pts3d, const float *pts2d,
                                                  Cam cam, float th2, const double *hyp, int *counts) {
  __shared__ float s3[kStage * 3], s2[kStage * 2];
  __shared__ int cnt[1024];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int o0 = offsets[p], n = offsets[p + 1] - o0;
  if (n <= kModel) return;  // (uniform over the block)
  for (int h = tid; h < iters; h += 256) cnt[h] = 0;
  for (int c0 = 0; c0 < n; c0 += kStage) {
    const int m = min(kStage, n - c0);
    __syncthreads();
    for (int i = tid; i < 3 * m; i += 256) s3[i] = pts3d[3 * (size_t)(o0 + c0) + i];
    for (int i = tid; i < 2 * m; i += 256) s2[i] = pts2d[2 * (size_t)(o0 + c0) + i];
    __syncthreads();
    for (int h = wave; h < iters; h += 4) {
      const double *T = hyp + ((size_t)p * iters + h) * 12;
      double Tr[12];
      for (int k = 0; k < 12; k++) Tr[k] = T[k];
      int good = 0;
      for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < m && pnp_inlier(Tr, s3[3 * i], s3[3 * i + 1], s3[3 * i + 2], s2[2 * i], s2[2 * i + 1], cam, th2);
        good += __popcll(__ballot(in));
      }
      if (lane == 0) cnt[h] += good;
    }
  }
  __syncthreads();
  for (int h = tid; h < iters; h += 256) counts[(size_t)p * iters + h] = cnt[h];
}

// RANSACUpdateNumIters (ptsetreg.cpp)
__host__ __device__ inline int update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = fmax(p, 0.), p = fmin(p, 1.);
  ep = fmax(ep, 0.), ep = fmin(ep, 1.);
  double num = fmax(1. - p, 2.2250738585072014e-308);  // DBL_MIN
  double denom = 1. - pow(1. - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// one lane per problem: the ordered loop of RANSACPointSetRegistrator::run, the winner's mask, status 1 / 0
__global__ __launch_bounds__(64) void k_pnp_replay(int P, int iters, double conf, const int *offsets, const float *pts3d,
                                                  const float *pts2d, Cam cam, float th2, const int *counts, const double *hyp,
                                                  uint8_t *mask, int *n_inl, int *status, int *best_iter, int *final_niters) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int o0 = offsets[p], n = offsets[p + 1] - o0;
  int best = -1, max_good = 0, niters = iters > 1 ? iters : 1;
  if (n < kModel) {
    for (int i = 0; i < n; i++) mask[o0 + i] = 0;
    n_inl[p] = 0, status[p] = 0, best_iter[p] = -1, final_niters[p] = 0;
    return;
  }
  if (n == kModel) {  // count == modelPoints: one solve on all five, all inliers
    for (int i = 0; i < n; i++) mask[o0 + i] = 1;
    n_inl[p] = n, status[p] = 1, best_iter[p] = -1, final_niters[p] = niters;
    return;
  }
  for (int it = 0; it < niters; it++) {
    const int good = counts[(size_t)p * iters + it];
    if (good > max(max_good, kModel - 1)) {
      best = it, max_good = good;
      niters = update_num_iters(conf, (double)(n - good) / n, kModel, niters);
    }
  }
  best_iter[p] = best, final_niters[p] = niters;
  if (best < 0) {
    for (int i = 0; i < n; i++) mask[o0 + i] = 0;
    n_inl[p] = 0, status[p] = 0;
    return;
  }
  const double *T = hyp + ((size_t)p * iters + best) * 12;
  int c = 0;
  for (int i = 0; i < n; i++) {
    const size_t k = o0 + i;
    const bool in = pnp_inlier(T, pts3d[3 * k], pts3d[3 * k + 1], pts3d[3 * k + 2], pts2d[2 * k], pts2d[2 * k + 1], cam, th2);
    mask[k] = in;
    c += in;
  }
  n_inl[p] = c, status[p] = 1;
}

__global__ void k_pnp_fill_fail(int P, const int *status, double *Tcw) {  // failed problems: zero pose
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < P && status[p] != 1)
    for (int k = 0; k < 12; k++) Tcw[12 * p + k] = 0.0;
}

// The intermediates of one call, carved from one workspace (the caller's in the _dev form: calls on different streams
// never share them).  Offsets aligned to 256 bytes.
struct PnpWs {
  int *samples, *counts, *best, *niters;
  double *hyp;
};
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t ws_bytes(int P, int iters) {
  const size_t H = (size_t)P * iters;
  return align256(H * kModel * 4) + align256(H * 12 * 8) + align256(H * 4) + 2 * align256((size_t)P * 4);
}
PnpWs ws_carve(void *w, int P, int iters) {
  const size_t H = (size_t)P * iters;
  char *c = (char *)w;
  PnpWs r;
  r.samples = (int *)c, c += align256(H * kModel * 4);
  r.hyp = (double *)c, c += align256(H * 12 * 8);
  r.counts = (int *)c, c += align256(H * 4);
  r.best = (int *)c, c += align256((size_t)P * 4);
  r.niters = (int *)c;
  return r;
}

int pnp_enqueue(int P, const int32_t *offsets, const float *pts3d, const float *pts2d, const float cam4[4], int iters,
                float reproj, double conf, double *Tcw, uint8_t *mask, int32_t *n_inl, int32_t *status, const vo_pnp_diag *diag,
                void *workspace, hipStream_t st) {
  const Cam cam{(double)cam4[0], (double)cam4[1], (double)cam4[2], (double)cam4[3]};
  const size_t H = (size_t)P * iters;
  const PnpWs w = ws_carve(workspace, P, iters);
  // hypotheses of problems with n <= 5 are never read; zeroed so that the diagnostics are defined
  VO_HIP_CHECK(hipMemsetAsync(w.samples, 0, H * kModel * 4, st));
  VO_HIP_CHECK(hipMemsetAsync(w.hyp, 0, H * 12 * 8, st));
  VO_HIP_CHECK(hipMemsetAsync(w.counts, 0, H * 4, st));
  const float th2 = (float)((double)reproj * (double)reproj);
  hipLaunchKernelGGL(k_pnp_samples, dim3((P + 63) / 64), dim3(64), 0, st, P, offsets, iters, w.samples);
  const int per = kEpnpBlock / kGroup;
  hipLaunchKernelGGL(k_pnp_epnp, dim3((unsigned)((H + per - 1) / per)), dim3(kEpnpBlock), 0, st, 0, P, iters, offsets, pts3d,
                     pts2d, cam, (const int *)w.samples, (uint8_t *)nullptr, (int *)nullptr, (int *)nullptr, w.hyp);
  hipLaunchKernelGGL(k_pnp_score, dim3(P), dim3(256), 0, st, iters, offsets, pts3d, pts2d, cam, th2, (const double *)w.hyp,
                     w.counts);
  hipLaunchKernelGGL(k_pnp_replay, dim3((P + 63) / 64), dim3(64), 0, st, P, iters, conf, offsets, pts3d, pts2d, cam, th2,
                     (const int *)w.counts, (const double *)w.hyp, mask, n_inl, status, w.best, w.niters);
  hipLaunchKernelGGL(k_pnp_epnp, dim3((P + per - 1) / per), dim3(kEpnpBlock), 0, st, 1, P, iters, offsets, pts3d, pts2d, cam,
                     (const int *)nullptr, mask, status, n_inl, Tcw);
  hipLaunchKernelGGL(k_pnp_fill_fail, dim3((P + 63) / 64), dim3(64), 0, st, P, status, Tcw);
  VO_HIP_CHECK(hipGetLastError());
  if (diag) {  // device copies (the host form passes its own staging)
    if (diag->samples) VO_HIP_CHECK(hipMemcpyAsync(diag->samples, w.samples, H * kModel * 4, hipMemcpyDefault, st));
    if (diag->counts) VO_HIP_CHECK(hipMemcpyAsync(diag->counts, w.counts, H * 4, hipMemcpyDefault, st));
    if (diag->hyp_Tcw12) VO_HIP_CHECK(hipMemcpyAsync(diag->hyp_Tcw12, w.hyp, H * 12 * 8, hipMemcpyDefault, st));
    if (diag->best_iter) VO_HIP_CHECK(hipMemcpyAsync(diag->best_iter, w.best, (size_t)P * 4, hipMemcpyDefault, st));
    if (diag->final_niters) VO_HIP_CHECK(hipMemcpyAsync(diag->final_niters, w.niters, (size_t)P * 4, hipMemcpyDefault, st));
  }
  return VO_OK;
}

int pnp_check(int P, int iters, float reproj, double conf, const float *cam4) {
  if (P < 0 || !cam4 || !(reproj >= 0) || !(conf > 0 && conf < 1)) return VO_ERR_INVALID;
  if (iters < 1) return VO_ERR_INVALID;
  if (P > VO_PNP_MAX_PROBLEMS || iters > VO_PNP_MAX_ITERATIONS || (long long)P * iters > VO_PNP_MAX_HYPOTHESES) {
    vo::set_error("vo_pnp_ransac: %d problems x %d iterations exceed the capacity (%d problems, %d iterations, %d hypotheses)", P,
                  iters, VO_PNP_MAX_PROBLEMS, VO_PNP_MAX_ITERATIONS, VO_PNP_MAX_HYPOTHESES);
    return VO_ERR_CAPACITY;
  }
  return VO_OK;
}

}  // namespace

extern "C" {

size_t vo_pnp_workspace_bytes(int n_problems, int iterations) {
  if (n_problems < 0 || iterations < 1) return 0;
  return ws_bytes(n_problems, iterations);
}

int vo_pnp_ransac_dev(int n_problems, const int32_t *offsets, const float *pts3d, const float *pts2d, const float cam4[4],
                      int iterations, float reproj_error, double confidence, double *Tcw12, uint8_t *inlier, int32_t *n_inliers,
                      int32_t *status, const vo_pnp_diag *diag, void *workspace, size_t workspace_bytes, void *hip_stream) {
  VO_CHECK(pnp_check(n_problems, iterations, reproj_error, confidence, cam4));
  if (n_problems == 0) return VO_OK;
  if (!offsets || !pts3d || !pts2d || !Tcw12 || !inlier || !n_inliers || !status || !workspace) return VO_ERR_INVALID;
  if (workspace_bytes < ws_bytes(n_problems, iterations)) {
    vo::set_error("vo_pnp_ransac_dev: workspace of %zu bytes, %zu needed (vo_pnp_workspace_bytes)", workspace_bytes,
                  ws_bytes(n_problems, iterations));
    return VO_ERR_CAPACITY;
  }
  VO_CHECK(vo::ensure_device());
  return pnp_enqueue(n_problems, offsets, pts3d, pts2d, cam4, iterations, reproj_error, confidence, Tcw12, inlier, n_inliers,
                     status, diag, workspace, (hipStream_t)hip_stream);
}

int vo_pnp_ransac(int n_problems, const int32_t *offsets, const float *pts3d, const float *pts2d, const float cam4[4],
                  int iterations, float reproj_error, double confidence, double *Tcw12, double *pose6, uint8_t *inlier,
                  int32_t *n_inliers, int32_t *status, const vo_pnp_diag *diag) {
  VO_CHECK(pnp_check(n_problems, iterations, reproj_error, confidence, cam4));
  if (n_problems == 0) return VO_OK;
  if (!offsets || !Tcw12 || !n_inliers || !status) return VO_ERR_INVALID;
  if (offsets[0] != 0) return VO_ERR_INVALID;
  for (int p = 0; p < n_problems; p++) {
    const long long n = (long long)offsets[p + 1] - offsets[p];
    if (n < 0) return VO_ERR_INVALID;
    if (n > VO_PNP_MAX_POINTS) {
      vo::set_error("vo_pnp_ransac: problem %d has %lld correspondences (capacity %d)", p, n, VO_PNP_MAX_POINTS);
      return VO_ERR_CAPACITY;
    }
  }
  const size_t N = (size_t)offsets[n_problems], P = n_problems, H = P * iterations;
  if (N > 0 && (!pts3d || !pts2d || !inlier)) return VO_ERR_INVALID;
  VO_CHECK(vo::ensure_device());
  thread_local vo::ScratchBuf d_off, d_p3, d_p2, d_T, d_m, d_ni, d_st, d_ws, g_s, g_c, g_h, g_b, g_n;
  hipStream_t st = vo::thread_stream();
  const char *W = "vo_pnp_ransac";
  VO_CHECK(vo::upload(d_off, offsets, (P + 1) * 4, st, W));
  VO_CHECK(d_p3.reserve(std::max<size_t>(N * 12, 16)));
  VO_CHECK(d_p2.reserve(std::max<size_t>(N * 8, 16)));
  if (N > 0) {
    VO_CHECK(vo::copy_h2d(d_p3.p, pts3d, N * 12, st, W));
    VO_CHECK(vo::copy_h2d(d_p2.p, pts2d, N * 8, st, W));
  }
  VO_CHECK(d_T.reserve(P * 96));
  VO_CHECK(d_m.reserve(std::max<size_t>(N, 16)));
  VO_CHECK(d_ni.reserve(P * 4));
  VO_CHECK(d_st.reserve(P * 4));
  VO_CHECK(d_ws.reserve(ws_bytes(n_problems, iterations)));  // (this thread's, used only inside this synchronous call)
  vo_pnp_diag dd{}, *pd = nullptr;
  if (diag) {
    if (diag->samples) {
      VO_CHECK(g_s.reserve(H * kModel * 4));
      dd.samples = g_s.as<int32_t>();
    }
    if (diag->counts) {
      VO_CHECK(g_c.reserve(H * 4));
      dd.counts = g_c.as<int32_t>();
    }
    if (diag->hyp_Tcw12) {
      VO_CHECK(g_h.reserve(H * 96));
      dd.hyp_Tcw12 = g_h.as<double>();
    }
    if (diag->best_iter) {
      VO_CHECK(g_b.reserve(P * 4));
      dd.best_iter = g_b.as<int32_t>();
    }
    if (diag->final_niters) {
      VO_CHECK(g_n.reserve(P * 4));
      dd.final_niters = g_n.as<int32_t>();
    }
    pd = &dd;
  }
  VO_CHECK(pnp_enqueue(n_problems, d_off.as<int32_t>(), d_p3.as<float>(), d_p2.as<float>(), cam4, iterations, reproj_error,
                       confidence, d_T.as<double>(), d_m.as<uint8_t>(), d_ni.as<int32_t>(), d_st.as<int32_t>(), pd, d_ws.p, st));
  VO_CHECK(vo::copy_d2h(Tcw12, d_T.p, P * 96, st, W));
  if (N > 0) VO_CHECK(vo::copy_d2h(inlier, d_m.p, N, st, W));
  VO_CHECK(vo::copy_d2h(n_inliers, d_ni.p, P * 4, st, W));
  VO_CHECK(vo::copy_d2h(status, d_st.p, P * 4, st, W));
  if (diag) {
    if (diag->samples) VO_CHECK(vo::copy_d2h(diag->samples, g_s.p, H * kModel * 4, st, W));
    if (diag->counts) VO_CHECK(vo::copy_d2h(diag->counts, g_c.p, H * 4, st, W));
    if (diag->hyp_Tcw12) VO_CHECK(vo::copy_d2h(diag->hyp_Tcw12, g_h.p, H * 96, st, W));
    if (diag->best_iter) VO_CHECK(vo::copy_d2h(diag->best_iter, g_b.p, P * 4, st, W));
    if (diag->final_niters) VO_CHECK(vo::copy_d2h(diag->final_niters, g_n.p, P * 4, st, W));
  }
  VO_CHECK(vo::stream_sync(st, W));
  if (pose6)
    for (size_t p = 0; p < P; p++) {
      const double *T = Tcw12 + 12 * p;
      const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
      if (status[p] == 1)
        VO_CHECK(vo_se3_log(R, t, pose6 + 6 * p));
      else
        for (int k = 0; k < 6; k++) pose6[6 * p + k] = 0.0;
    }
  return VO_OK;
}

}  // extern "C"
